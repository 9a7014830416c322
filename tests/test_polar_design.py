"""BEC design of polar codes over mixed kernels (csrc/polar_design.cpp): the capacity evaluation
of a kernel's BEC table (CBECCapacityEvaluator::GetSubchannelCapacity restated, out/external/
CapacityEvaluator.cpp:124-140 -- parity unpinned: the reference's evaluator needs GSL and is never
built), the kernel-file writer (Kernel.cpp:93-134) and bchk_polar_design_bec's layer recursion,
tied to the encoder by composing the layers into one big kernel and enumerating that on the GPU."""
import ctypes as C
import os
from math import comb

import numpy as np
import pytest

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
    """A matrix layer whose file carries the table needs no GPU; the capacities are the table's."""
    b = load()
    tab = table_of(b.kernel_ebch(2))
    spec, cap = b.design_bec(["-k4t.txt", "A"], 4, 0.4, kernel_dir=kdir)
    want = []
    for a0 in range(4):
        t = b.kernel_bec_capacity(tab, a0, 0.4)
        want += [t * t, 2 * t - t * t]
    assert cap.tolist() == want
    o = PolarOracle(spec, kdir)
    assert (o.N, o.K) == (8, 4)


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
