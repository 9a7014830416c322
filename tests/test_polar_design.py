"""BEC design of polar codes over mixed kernels (csrc/polar_design.cpp): the capacity evaluation
of a kernel's BEC table (CBECCapacityEvaluator::GetSubchannelCapacity restated, out/external/
CapacityEvaluator.cpp:124-140) and the kernel-file writer (Kernel.cpp:93-134), both pinned to the
compiled reference by tests/golden/polar_ref_capacity_*.txt.gz (its reader loaded the files our
writer wrote; its evaluator's outputs are recorded, NaN and -inf included), and
bchk_polar_design_bec's layer recursion, tied to the encoder by composing the layers into one big
kernel and enumerating that on the GPU, and to an exact rational recursion for deep designs."""
import ctypes as C
import math
import os
from fractions import Fraction
from math import comb

import numpy as np
import pytest

import polar_ref_lib as R
from bchk_pkg import load
from bec_lib import erasure_polynomial, histogram, np_masks
from polar_lib import PolarOracle

F2 = np.array([[1, 0], [1, 1]], np.uint8)
ARIKAN_TABLE = np.array([[0, 2, 1], [0, 0, 1]], np.uint64)


def table_of(K):
    """The exact BEC table of a small kernel from the numpy checker."""
    l = len(K)
    pat = np.arange(1 << l, dtype=np.uint64)
    return histogram(l, pat, np_masks(K, pat))


@pytest.fixture(scope="module")
def kdir(tmp_path_factory):
    """Kernel files written by write_kernel_file: the 4 x 4 and 16 x 16 extended-BCH kernels with
    their tables (so designs over them need no GPU) and without."""
    b = load()
    d = tmp_path_factory.mktemp("bec_kernels")
    for name, power in (("k4", 2), ("e16", 4)):
        K = b.kernel_ebch(power)
        b.write_kernel_file(os.path.join(d, name + ".txt"), K)
        b.write_kernel_file(os.path.join(d, name + "t.txt"), K, table_of(K))
    return str(d)


# ---- host

def test_capacity_matches_the_reference_loop():
    b = load()
    tab = table_of(b.kernel_ebch(4))
    l = 16
    for cap in np.linspace(0.05, 0.95, 10):
        for ph in range(l):
            P, S, E = 1 - cap, (1 - cap) / cap, 0.0
            for i in range(l, 0, -1):  # CapacityEvaluator.cpp:131-139
                E *= S
                E += float(tab[ph, i])
            E *= S * cap ** l
            got = b.kernel_bec_capacity(tab, ph, float(cap))
            assert abs(got - (1 - E)) <= 1e-15, (ph, cap)
            assert abs(got - float(1 - erasure_polynomial(tab[ph], l, 1 - float(cap)))) <= 1e-12
    for ph in range(l):
        assert b.kernel_bec_capacity(tab, ph, 0.0) == 0.0
        assert b.kernel_bec_capacity(tab, ph, 1.0) == 1.0
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(b.BchkError):
            b.kernel_bec_capacity(tab, 0, bad)
    with pytest.raises(b.BchkError):
        b.kernel_bec_capacity(tab, 16, 0.5)


def test_capacity_of_the_arikan_table():
    b = load()
    for cap in np.linspace(0.0, 1.0, 21):
        cap = float(cap)
        assert abs(b.kernel_bec_capacity(ARIKAN_TABLE, 0, cap) - cap * cap) <= 1e-15
        assert abs(b.kernel_bec_capacity(ARIKAN_TABLE, 1, cap) - (2 * cap - cap * cap)) <= 1e-15


def test_kernel_file_round_trip(tmp_path):
    b = load()
    K = b.kernel_ebch(4)
    tab = table_of(K)
    path = os.path.join(tmp_path, "e16.txt")
    b.write_kernel_file(path, K, tab)
    tok = open(path).read().split()
    assert int(tok[0]) == 16
    assert np.array_equal(np.array(tok[1:257], np.uint8).reshape(16, 16), K)
    assert tok[257] == "3"  # ec_BEC
    rows = np.array([int(t) for t in tok[258:]], dtype=object).reshape(16, 17)
    assert all(r[0] == 0 for r in rows)  # the constructor insists on it (CapacityEvaluator.cpp:107)
    assert [[int(v) for v in r[1:]] for r in rows] == [[int(v) for v in r[1:]] for r in tab]
    b.write_kernel_file(os.path.join(tmp_path, "plain.txt"), K)
    assert open(os.path.join(tmp_path, "plain.txt")).read().split() == tok[:257]
    # both load as kernels: what follows the matrix is ignored
    for name in ("-e16.txt", "-plain.txt"):
        o = PolarOracle(f"16 16 0 1 0 0\n{name}\n", str(tmp_path))
        assert (o.N, o.K) == (16, 16)
        assert np.array_equal(o.encode(np.eye(16, dtype=np.uint8)), K)
    with pytest.raises(b.BchkError):
        b.write_kernel_file(os.path.join(tmp_path, "no", "such", "dir.txt"), K)


def classical_bec(n, cap):
    """Capacities of the 2^n symbols of the Arikan code in the decoder's index order: the most
    significant index bit transforms the channel itself."""
    c = [cap]
    for _ in range(n):
        c = [f for x in c for f in (x * x, 2 * x - x * x)]
    return c


def frozen_of(spec):
    lines = spec.strip().split("\n")
    fr = [tuple(int(t) for t in ln.split()) for ln in lines[2:]]
    assert all(len(f) == 2 and f[0] == 1 for f in fr)
    return lines[0], lines[1], [f[1] for f in fr]


def test_design_all_arikan_is_the_classical_construction():
    b = load()
    n, K = 10, 512
    spec, cap = b.design_bec(["A"] * n, K, 0.5)
    want = classical_bec(n, 0.5)
    assert cap.tolist() == want
    order = sorted(range(1 << n), key=lambda i: (want[i], i), reverse=True)  # ties: higher index first
    head, layers, frozen = frozen_of(spec)
    assert head == f"{1 << n} {K} 0 {n} 0 0" and layers == " ".join(["A"] * n)
    assert frozen == sorted(order[K:])
    o = PolarOracle(spec)
    assert (o.N, o.K, o.U) == (1 << n, K, 1 << n)


def test_design_ties_go_to_the_higher_index(kdir):
    b = load()
    for layers, U in ((["A"] * 4, 16), (["-k4t.txt", "A"], 8)):
        for cap in (0.0, 1.0):  # every symbol ties
            spec, c = b.design_bec(layers, 5, cap, kernel_dir=kdir)
            assert set(c.tolist()) == {cap}
            assert frozen_of(spec)[2] == list(range(U - 5))
    spec, c = b.design_bec("A", 1, 0.0)
    assert frozen_of(spec)[2] == [0]


def test_design_uses_the_file_table(kdir):
    """A matrix layer whose file carries the table needs no GPU; the capacities are the table's:
    the exact polynomial in Fractions, under the bound of error_bounds (below)."""
    b = load()
    tab = table_of(b.kernel_ebch(2))
    spec, cap = b.design_bec(["-k4t.txt", "A"], 4, 0.4, kernel_dir=kdir)
    want = []
    for a0 in range(4):
        t = 1 - erasure_polynomial(tab[a0], 4, 1 - Fraction(0.4))
        want += [t * t, 2 * t - t * t]
    rho, floor = error_bounds(["-k4t.txt", "A"], 0.0)
    assert rho < 1e-14
    for got, w in zip(cap.tolist(), want):
        assert abs(Fraction(got) - w) <= Fraction(rho) * w + Fraction(floor), (got, float(w))
    o = PolarOracle(spec, kdir)
    assert (o.N, o.K) == (8, 4)


# ---- the evaluator and the writer against the compiled reference

CAPACITY_FILES = R.fixture_files("capacity")
_cap_ids = lambda p: os.path.basename(p)[len("polar_ref_capacity_"):-len(".txt.gz")]  # noqa: E731
GRID_EXACT = {"bch4": 84, "bch16": 336, "kron5": 672}  # measured: every grid value, DESIGN.md section 9


def capacity_fixture(path):
    """(kernel-file name, its text, l, K, table [l][l + 1] as written, capacities, recorded [n][l])."""
    fx = R.load_fixture(path)
    fname, text = fx.kernel_file
    tok = text.split()
    l = int(tok[0])
    K = np.array(tok[1:1 + l * l], np.uint8).reshape(l, l)
    assert tok[1 + l * l] == "3"
    tab = np.array([int(t) for t in tok[2 + l * l:]], np.uint64).reshape(l, l + 1)
    caps = [float(R.f64_row(r)[0]) for r in fx.get("capacity_in")]
    want = np.array([R.f64_row(r) for r in fx.get("capacity_out")])
    return fname, text, l, K, tab, caps, want


def test_the_capacity_fixture_set_is_the_one_the_generator_writes():
    assert sorted(_cap_ids(p) for p in CAPACITY_FILES) == sorted(GRID_EXACT)
    for p in CAPACITY_FILES:
        _, _, l, _, _, caps, want = capacity_fixture(p)
        assert caps == [round(0.05 * i, 2) for i in range(1, 20)] + [1 - 1e-9, 1.0, 1e-3, 1e-5, 1e-10, 1e-20, 1e-40, 0.0]
        assert want.shape == (len(caps), l)
    # the rows that document where the reference's rule stops working are really there
    _, _, _, _, _, caps, want = capacity_fixture(os.path.join(R.GOLD, "polar_ref_capacity_bch16.txt.gz"))
    assert np.isnan(want[caps.index(1e-40)]).any() and np.isnan(want[caps.index(0.0)]).all()
    assert (want[caps.index(1e-5)] < 0).any()


@pytest.mark.parametrize("path", CAPACITY_FILES, ids=_cap_ids)
def test_capacity_matches_the_compiled_reference(path):
    """The same Horner rule, both built without contraction: equal bits expected. On the grid
    0.05 .. 1.0 the only freedom is the last place of pow between C libraries, on an E <= 1:
    |difference| <= 2^-52, and the count of exact matches is the one measured (all of them). Below
    the grid (1e-3 .. 1e-40) the rule's own cancellation, overflow and NaN are reproduced bit for
    bit (NaN-aware). At C = 0 the reference divides by zero (NaN); the product documents
    1 - counts[phase][l] there (include/bchk.h), which is 0 for every table."""
    b = load()
    _, _, l, _, tab, caps, want = capacity_fixture(path)
    exact = 0
    for c, w in zip(caps, want):
        got = np.array([b.kernel_bec_capacity(tab, ph, c) for ph in range(l)])
        same = got.view(np.uint64) == w.view(np.uint64)
        print(_cap_ids(path), c, "equal bits:", int(same.sum()), "of", l)
        if c >= 0.05:
            exact += int(same.sum())
            assert np.all(np.abs(got - w) <= 2.0 ** -52), (c, got, w)
        elif c > 0.0:
            assert np.all(same | (np.isnan(got) & np.isnan(w))), (c, got, w)
        else:
            assert np.isnan(w).all()
            assert got.tolist() == [1.0 - float(tab[ph, l]) for ph in range(l)] == [0.0] * l
    assert exact == GRID_EXACT[_cap_ids(path)] == 21 * l


@pytest.mark.parametrize("path", CAPACITY_FILES, ids=_cap_ids)
def test_capacity_fixture_regenerates_byte_for_byte(path, tmp_path):
    if R.ref_lacks("capacity"):
        pytest.skip(R.ref_lacks("capacity"))
    fx = R.load_fixture(path)
    again = R.regenerate(fx, str(tmp_path))
    assert again.dumps() == fx.dumps()
    out = tmp_path / "again.txt.gz"
    again.save(str(out))
    assert out.read_bytes() == open(path, "rb").read()


def test_reference_reader_rejects_a_file_without_a_table(tmp_path):
    """polar_ref capacity exits 2 when the reader kept no BEC evaluator (it only warns)."""
    if R.ref_lacks("capacity"):
        pytest.skip(R.ref_lacks("capacity"))
    b = load()
    K = b.kernel_ebch(2)
    b.write_kernel_file(os.path.join(tmp_path, "plain.txt"), K)
    tab = table_of(K)
    tab[2, 0] = 1  # the constructor insists on a 0 there (CapacityEvaluator.cpp:107); our writer always writes one
    b.write_kernel_file(os.path.join(tmp_path, "tab.txt"), K, tab)
    assert R.run_ref(["capacity", "tab.txt"], [R.hex64(0.5)], str(tmp_path))
    with pytest.raises(RuntimeError, match="exit 2"):
        R.run_ref(["capacity", "plain.txt"], [R.hex64(0.5)], str(tmp_path))
    bad = open(os.path.join(tmp_path, "tab.txt")).read().split("\n")
    bad[7] = "1" + bad[7][1:]
    open(os.path.join(tmp_path, "bad.txt"), "w").write("\n".join(bad))
    with pytest.raises(RuntimeError, match="exit 2"):
        R.run_ref(["capacity", "bad.txt"], [R.hex64(0.5)], str(tmp_path))


def test_written_file_is_the_text_the_reference_loaded():
    """The writer on the CPU-side tables (the GPU tables: test_gpu_table_writes_the_file...)."""
    b = load()
    for p in CAPACITY_FILES:
        fname, text, l, K, tab, _, _ = capacity_fixture(p)
        if l <= 16:
            assert np.array_equal(K, b.kernel_ebch({4: 2, 16: 4}[l])) and np.array_equal(tab, table_of(K))


# ---- deep designs against the exact recursion

U53 = 2.0 ** -53      # unit roundoff
TINY = 2.0 ** -1074   # the smallest subnormal: bounds the absolute rounding error once a value underflows

DEEP_CASES = {
    "A8_e16": ["A"] * 8 + ["-e16t.txt"],
    "e16_e16": ["-e16t.txt"] * 2,
    "e16_e16_e16": ["-e16t.txt"] * 3,
    "k4x7": ["-k4t.txt"] * 7,
    "A_k4_A_e16": ["A", "-k4t.txt", "A", "-e16t.txt"],
}
DEEP_CAPACITIES = {"0.5": (0.5, Fraction(1, 2), 0.0), "0.1": (0.1, Fraction(1, 10), U53)}  # value, truth's input, its relative distance


def layer_size(name):
    return 2 if name == "A" else {"-k4t.txt": 4, "-e16t.txt": 16}[name]


def error_bounds(layers, rho0):
    """(rho, floor): |computed - exact| <= rho exact + floor for every symbol capacity of the
    design recursion, derived from the evaluator's operations, not from its output.

    One layer maps a capacity C to T(C) = sum_w d_w (1 - C)^w C^(l-w), d_w >= 0 (d_w = C(l, w)
    minus the table, the correctable patterns), T increasing from T(0) = 0 to T(1) = 1.
      Condition. T(C) / C^l = sum_w d_w ((1 - C) / C)^w falls as C grows, so 0 <= C T'(C) / T(C)
      <= l: the relative condition number is at most l, and an input within a factor (1 + r)
      gives an output within (1 + r)^l. In Bernstein form the coefficients d_w / C(l, w) lie in
      [0, 1], so |T'| <= l as well: an absolute input error a gives at most l a.
      Evaluation (csrc/polar_design.cpp design_row). P = 1 - C (1 rounding), the ratio of the
      smaller to the larger of P and C (1 more, so 2 on the ratio), Horner with l multiplications
      by it (3 each on the term that passes through all of them) and l additions of non-negative
      terms (1 each), the power of the larger (its base's rounding l times, pow itself at most 2),
      the final product (1): at most (3 l + l + l + 3) = (5 l + 3) roundings on any term, none
      amplified because no term is negative. Taken as (5 l + 4) u, u = 2^-53. The d_w are exact
      integers below 2^53. Once a partial result is subnormal each of the at most l + 1 roundings
      costs TINY absolutely instead.
      Arikan layers: C^2 (condition 2, 1 rounding), 2 C - C^2 = C (2 - C) >= C^2 (condition <= 1;
      the square's rounding and the subtraction's, each at most u of the result): l = 2, 2 u.
    So per layer rho <- (1 + rho)^l (1 + eps_l) - 1 and floor <- l floor + (l + 1) TINY, from
    rho0 = the relative distance of the design capacity from the truth's input; last, the exact
    value's own rounding to double (u, TINY). For values above 1/2 the relative bound is an
    absolute one, T being at most 1. Worst case over the five deep cases: 1.3e-11 (k4 x 7)."""
    rho, floor = rho0, 0.0
    for name in layers:
        l = layer_size(name)
        eps = 2 * U53 if name == "A" else (5 * l + 4) * U53
        rho = math.expm1(l * math.log1p(rho) + math.log1p(eps))
        floor = l * floor + (l + 1) * TINY
    return rho + U53, floor + TINY


_tables = {}


def int_table(name):
    if name not in _tables:
        tab = table_of(load().kernel_ebch({"-k4t.txt": 2, "-e16t.txt": 4}[name]))
        _tables[name] = [[int(v) for v in row] for row in tab]
    return _tables[name]


def exact_design(layers, c0):
    """The layer recursion of bchk_polar_design_bec in exact rational arithmetic: numerators over
    the common denominator den (every capacity at depth j is a Fraction with denominator
    c0.denominator ^ (l_0 .. l_{j-1}); kept unreduced, which is what makes 16384 symbols cheap).
    A matrix layer is the exact polynomial 1 - sum_w u[w] P^w C^(l-w) = sum_w (C(l, w) - u[w])
    P^w C^(l-w), u[0] = 0 as the file stores it."""
    nums, den = [c0.numerator], c0.denominator
    for name in layers:
        if name == "A":
            nums = [v for n in nums for v in (n * n, 2 * n * den - n * n)]
            den = den * den
            continue
        tab = int_table(name)
        l = len(tab)
        cor = [[comb(l, w) - (row[w] if w else 0) for w in range(l + 1)] for row in tab]
        assert all(v >= 0 for row in cor for v in row)
        out = []
        for n in nums:
            q = den - n
            pn, pq = [1], [1]
            for _ in range(l):
                pn.append(pn[-1] * n)
                pq.append(pq[-1] * q)
            terms = [pq[w] * pn[l - w] for w in range(l + 1)]
            for d in cor:
                out.append(sum(dw * t for dw, t in zip(d, terms) if dw))
        nums, den = out, den ** l
    return nums, den


_exact = {}


def exact_case(case, capname):
    """(numerators, denominator, the exact capacities rounded to double, the exact ranking: best
    first, ties to the higher index) -- computed once per case."""
    key = (case, capname)
    if key not in _exact:
        nums, den = exact_design(DEEP_CASES[case], DEEP_CAPACITIES[capname][1])
        f = [n / den for n in nums]  # int / int is correctly rounded, and 0.0 below the subnormals
        order = sorted(range(len(nums)), key=lambda i: (nums[i], i), reverse=True)
        _exact[key] = (nums, den, f, order)
    return _exact[key]


def test_exact_recursion_is_the_fraction_recursion():
    """The common-denominator integers against the literal recursion in fractions.Fraction."""
    layers = DEEP_CASES["A_k4_A_e16"]
    for c0 in (Fraction(1, 2), Fraction(1, 10)):
        c = [c0]
        for name in layers:
            if name == "A":
                c = [v for x in c for v in (x * x, 2 * x - x * x)]
            else:
                tab = int_table(name)
                c = [1 - erasure_polynomial([0] + row[1:], len(tab), 1 - x) for x in c for row in tab]
        nums, den = exact_design(layers, c0)
        assert [Fraction(n, den) for n in nums] == c


def separated_cut(f, order, target, rho, floor):
    """The K nearest to target at which the exact capacities on the two sides of the cut are
    further apart than the evaluator's error can bridge (from the exact values alone)."""
    U = len(order)
    for step in range(U):
        for K in (target - step, target + step):
            if 0 < K < U:
                hi, lo = f[order[K - 1]], f[order[K]]
                if hi * (1 - 2 * rho) - 2 * floor > lo * (1 + 2 * rho) + 2 * floor:
                    return K
    raise AssertionError("no separated cut")


@pytest.mark.parametrize("capname", list(DEEP_CAPACITIES))
@pytest.mark.parametrize("case", list(DEEP_CASES))
def test_deep_design_matches_the_exact_recursion(kdir, case, capname):
    """Matrix layers that are not the first see capacities down to 1e-77 and below, where the
    reference's Horner rule in (1 - C) / C overflows, cancels and returns NaN (the recorded rows
    of polar_ref_capacity_*): every capacity must be finite, in [0, 1] and within error_bounds of
    the exact value (relative up to 1/2, absolute above), and the frozen set must be the exact
    recursion's, at a rate near the capacity and at a high rate whose cut falls among symbols of
    capacity far below 1e-16.

    At the parent commit (the Horner rule in every matrix layer) all ten cases failed: NaN
    capacities in A8_e16 (128 at 0.5, 1216 at 0.1); negative capacities in every case (6 .. 677
    symbols); capacities of 1e-41 .. 1e-78 returned as +-1e-15, relative errors 1e18 .. 1e307; the
    high-rate frozen set wrong in every case (2 .. 3060 symbols) and the one near capacity wrong
    by 748 symbols in A8_e16 at 0.1."""
    b = load()
    layers = DEEP_CASES[case]
    c_float, _, rho0 = DEEP_CAPACITIES[capname]
    nums, den, f, order = exact_case(case, capname)
    U = len(nums)
    rho, floor = error_bounds(layers, rho0)
    assert rho < 2e-11
    _, cap = b.design_bec(layers, U // 2, c_float, kernel_dir=kdir)
    assert len(cap) == U and np.isfinite(cap).all() and (cap >= 0).all() and (cap <= 1).all()
    want = np.array(f)
    err = np.abs(cap - want)
    small = want <= 0.5
    rel = float(np.max(err[small & (want > 0)] / want[small & (want > 0)], initial=0.0))
    print(case, capname, "bound", rho, "worst relative error", rel, "worst absolute error above 1/2",
          float(np.max(err[~small], initial=0.0)), "smallest positive capacity", want[want > 0].min())
    assert np.all(err[small] <= rho * want[small] + floor)
    assert np.all(err[~small] <= rho)
    # frozen sets: near the capacity, and a high rate that ranks the tiny capacities
    deep_target = int(np.sum(want > 1e-40))
    cuts = [separated_cut(f, order, max(1, round(U * c_float)), rho, floor),
            separated_cut(f, order, deep_target, rho, floor)]
    assert f[order[cuts[1]]] < 1e-30 and f[order[cuts[1] - 1]] > 1e-300 and cuts[1] > cuts[0]
    for K in cuts:
        spec, _ = b.design_bec(layers, K, c_float, kernel_dir=kdir)
        head, line, frozen = frozen_of(spec)
        assert head == f"{U} {K} 0 {len(layers)} 0 0" and line == " ".join(layers)
        assert frozen == sorted(order[K:]), (case, capname, K)


def test_design_bad_input(kdir):
    b = load()
    L = b.lib()

    def call(layers, K, cap=0.5, room=1 << 16):
        buf = C.create_string_buffer(max(room, 1))
        needed = C.c_size_t(12345)
        rc = L.bchk_polar_design_bec(layers.encode(), kdir.encode(), K, cap, 1 << 12, 1, 0, None, buf, room,
                                     C.byref(needed))
        return rc, needed.value, buf.value.decode()

    rc, needed, text = call("A A A", 4)
    assert rc == 0 and needed == len(text) + 1 and text.startswith("8 4 0 3 0 0\nA A A\n1 ")
    assert call("A A A", 9)[:2] == (-1, 0)            # K > U
    assert call("A A A", -1)[:2] == (-1, 0)
    assert call("A B A", 4)[:2] == (-1, 0)            # unknown kernel
    assert call("A -missing.txt", 4)[:2] == (-1, 0)   # no such file
    assert call("", 0)[:2] == (-1, 0)
    assert call("A A A", 4, cap=1.5)[:2] == (-1, 0)
    assert call("A A A", 4, room=needed - 1)[:2] == (-1, needed)  # short buffer: needed is set
    assert call("A A A", 4, room=needed)[0] == 0
    with pytest.raises(b.BchkError, match="Unknown kernel"):
        b.design_bec("A Q", 1)
    open(os.path.join(kdir, "sing.txt"), "w").write("2\n1 1\n1 1\n")
    with pytest.raises(b.BchkError, match="singular"):
        b.design_bec("-sing.txt A", 1, kernel_dir=kdir)


# ---- GPU

@pytest.mark.gpu
def test_written_files_and_designed_specs_load_on_the_gpu(kdir):
    b = load()
    d = b.PolarListDecoder("16 16 0 1 0 0\n-e16t.txt\n", 1, kernel_dir=kdir)
    assert (d.N, d.K) == (16, 16)
    assert np.array_equal(d.encode(np.eye(16, dtype=np.uint8)), b.kernel_ebch(4))
    spec, _ = b.design_bec(["A"] * 10, 512, 0.5)
    d = b.PolarListDecoder(spec, 4)
    assert (d.N, d.K, d.U) == (1024, 512, 1024)
    # a file without a table: the GPU computes it, and the design equals the one from the table
    with_tab = b.design_bec(["-e16t.txt", "A"], 16, 0.5, kernel_dir=kdir)
    without = b.design_bec(["-e16.txt", "A"], 16, 0.5, kernel_dir=kdir)
    assert np.array_equal(with_tab[1], without[1])
    assert frozen_of(with_tab[0])[2] == frozen_of(without[0])[2]


@pytest.mark.gpu
@pytest.mark.parametrize("path", [p for p in CAPACITY_FILES if _cap_ids(p) != "bch4"],
                         ids=[i for i in map(_cap_ids, CAPACITY_FILES) if i != "bch4"])
def test_gpu_table_writes_the_file_the_reference_loaded(path, tmp_path):
    """kernel_bec_behaviour's table (all 2^32 patterns for the 32 x 32 Kronecker power) through
    write_kernel_file: byte for byte the text the reference's reader parsed for the fixture."""
    b = load()
    fname, text, l, K, _, _, _ = capacity_fixture(path)
    out = os.path.join(tmp_path, fname)
    b.write_kernel_file(out, K, b.kernel_bec_behaviour(K))
    assert open(out, "rb").read() == text.encode()


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [("-k4.txt", "A"), ("A", "-k4.txt"), ("A", "-k4.txt", "-k4t.txt")],
                         ids=lambda l: "_".join(l))
def test_recursion_matches_the_composed_kernel(kdir, layers):
    """The U x U generator (unit vectors through the encoder of a K = U spec) taken as one kernel
    of size U: its exact erasure polynomial per row must be what the layer recursion gives."""
    b = load()
    size = {"A": 2, "-k4.txt": 4, "-k4t.txt": 4}
    U = int(np.prod([size[n] for n in layers]))
    d = b.PolarListDecoder(f"{U} {U} 0 {len(layers)} 0 0\n{' '.join(layers)}\n", 1, kernel_dir=kdir)
    G = d.encode(np.eye(U, dtype=np.uint8))
    counts = b.kernel_bec_behaviour(G)
    assert [int(sum(int(v) for v in counts[:, w])) for w in range(U + 1)] == [w * comb(U, w) for w in range(U + 1)]
    for capacity in (0.3, 0.5, 0.8):
        _, cap = b.design_bec(layers, U // 2, capacity, kernel_dir=kdir)
        for i in range(U):
            want = 1.0 - float(erasure_polynomial(counts[i], U, 1 - capacity))  # exact in the counts
            assert abs(cap[i] - want) <= 1e-12, (i, capacity, cap[i], want)


@pytest.mark.gpu
def test_design_over_the_64_kernel_uses_the_sampled_table(kdir):
    """Above 32 the table is bchk_kernel_bec_sample's estimate unc C(l, w) / tried."""
    b = load()
    K = b.kernel_ebch(6)
    b.write_kernel_file(os.path.join(kdir, "e64.txt"), K)
    spec, cap = b.design_bec(["-e64.txt"], 32, 0.5, kernel_dir=kdir, samples=1 << 12, seed=3)
    unc, tried, _ = b.kernel_bec_sample(K, 1 << 12, seed=3)
    for i in range(64):
        erased = sum(int(unc[i, w]) * comb(64, w) / int(tried[w]) for w in range(65)) / 2.0 ** 64
        assert abs(cap[i] - (1.0 - erased)) <= 1e-9, (i, cap[i], erased)
    assert cap[0] < 0.01 and cap[63] > 0.99
    head, _, frozen = frozen_of(spec)
    assert head == "64 32 0 1 0 0" and len(frozen) == 32
    assert frozen == sorted(np.argsort(cap, kind="stable")[:32].tolist())  # ties: the lower index is frozen


DESIGN_LAYERS = ("-e16.txt", "A", "A", "A")
DESIGN_K, DESIGN_L, DESIGN_SNR, DESIGN_WORDS, DESIGN_SEED = 64, 8, 3.0, 1 << 14, 11


def lowest_frozen_spec(layers, K):
    U = 16 * 2 ** (len(layers) - 1)
    return f"{U} {K} 0 {len(layers)} 0 0\n{' '.join(layers)}\n" + "".join(f"1 {f}\n" for f in range(U - K))


@pytest.mark.gpu
def test_designed_code_beats_lowest_indices_frozen(kdir):
    """The same 2^14 words of the same stream through both codes: the designed one must show
    strictly fewer block errors. Counts measured on the MI355X and the CPU pre-check (PolarOracle)
    that shows the margin: DESIGN.md."""
    b = load()
    spec, _ = b.design_bec(DESIGN_LAYERS, DESIGN_K, 0.5, kernel_dir=kdir)
    errors = {}
    for name, s in (("designed", spec), ("lowest", lowest_frozen_spec(DESIGN_LAYERS, DESIGN_K))):
        d = b.PolarListDecoder(s, DESIGN_L, kernel_dir=kdir)
        recs, _, _ = d.sweep_device(DESIGN_SNR, 0.5, 1, DESIGN_WORDS, 10 ** 9, seed=DESIGN_SEED)
        assert recs[0][1][0] == DESIGN_WORDS
        errors[name] = recs[0][1][1]
        d.close()
    print("block errors over", DESIGN_WORDS, "words at", DESIGN_SNR, "dB:", errors)
    assert errors["lowest"] >= 200
    assert errors["designed"] < errors["lowest"]
