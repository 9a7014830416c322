"""The int8 SC-list kernels (csrc/polar_sclist_q8.hip, csrc/polar_sclist_q8_tiered.hip) held to the
contract tests of the f32 kernels: what tests/test_polar_contract.py and
tests/test_polar_dense_dyn.py pin for the f32 decoders, through an llr="q8" context in the LDS
state and in the tiered state at every split, and through both entry points
(bchk_polar_decode_q8_host, bchk_polar_decode_q8_device). tests/test_polar_q8*.py decode through
PolarListDecoder.decode only -- zero-filled outputs, always a codeword buffer -- and with at most
eight dynamic constraints; here

  outputs hold a sentinel, device buffers lie between guard bytes: a write to a list row at or
    past the count, or outside a buffer, fails (lists shorter than L, three workgroups reusing
    their state over 70 words);
  cw = NULL / d_cw = 0 at both codeword store shapes;
  the epilogue's packed and byte stores at every (K mod 4, N mod 4), K past a record word and past
    a lane round (K = 264: 66 packed information stores);
  K = 0 and K = U;
  dense dynamic freezing (33 and 64 constraints live at once: the high word of PathRegs::dm, and
    the tiered kernel's lazy-copy tier around clone_regs' 64-bit copy);
  the genie calls on an int8 context, alone and between int8 decodes that share its buffers.

The reference is tests/sclist_q8.py through test_polar_q8.restated, compared bit for bit by
test_polar_contract.assert_strict: counts, information rows, codeword rows, metric bits, and the
sentinel in every row past the count. The restatement is itself pinned here, on the CPU, to the C
oracle on the dense codes and on the edge codes (tests/test_polar_q8_plain.py pins it at four
constraints or fewer), with rows that cannot saturate. Three exceptions, where the claim IS an
equality of two call forms or two states: cw = NULL against the call with a buffer, the tiered
state's 96 dense rows against the LDS state's (whose first 16 are the restatement's), and the
genie on an int8 context against an f32 one.

Mutations these tests were seen to catch (on a scratch copy): a 0.0f stored to the
metric rows [count, L) by test_gpu_q8_short_lists_leave_the_other_rows_and_the_guards; the packed
information loop cut to one lane round by test_gpu_q8_epilogue_store_shapes at K = 264; clone_regs
copying the low word of dm only by test_gpu_q8_dense_dynamic_freezing.

Wall time per test function on an MI355X, all cases of a parametrised one together and the CPU
restatement included (each test prints its own; the first GPU test of a process also loads the
library and starts the device, 1.7 s of its figure):

  test_gpu_q8_short_lists_leave_the_other_rows_and_the_guards  1.95 s  (3 cases, 0.09 s without the start)
  test_gpu_q8_cw_null                                          0.45 s  (5 cases)
  test_gpu_q8_epilogue_store_shapes                            1.15 s  (12 cases, at most 0.30 s)
  test_gpu_q8_dimension_zero_and_nothing_frozen                0.03 s  (2 cases)
  test_gpu_q8_dense_dynamic_freezing                           3.92 s  (7 cases, at most 1.37 s: L = 32 at U = 256)
  test_gpu_q8_genie_on_int8_contexts                           0.15 s  (2 cases)

and 1.7 s for the sixteen CPU tests.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import dense_codes
import sclist_q8
from bchk_pkg import load
from polar_lib import PolarOracle, arikan_spec
from test_polar_contract import (EDGE_K, NULL_CW_SPECS, SHORT_LISTS, STORES, Guarded, assert_strict, header,  # noqa: F401
                                 kdir, sentinel_outputs, short_spec)
from test_polar_dense_spec import direct_encode
from test_polar_q8 import assert_same, noisy_rows, restated


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print(f"\nwall time {request.node.name}: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------- contexts, entry points

def q8_states(spec, splits=None):
    """(label, state, split) of every way an int8 context keeps this code's state: the LDS state
    and the tiered one at every split 1..n (or at `splits`)."""
    n = header(spec)[2]
    return [("q8-lds", "lds", None)] + [(f"tiered_q8-{s}", "tiered_q8", s) for s in splits or range(1, n + 1)]


class q8_context:
    def __init__(self, spec, L, state="lds", split=None):
        self.d = load().PolarListDecoder(spec, L, llr="q8", state=state, split=split)
        assert self.d.split == (split or 0)

    def __enter__(self):
        return self.d

    def __exit__(self, *a):
        self.d.close()


def decode_q8_host(d, rows, cw=True):
    """bchk_polar_decode_q8_host on sentinel-filled outputs (cw=False: cw = NULL, the array returned
    is one the library never saw)."""
    rows = np.ascontiguousarray(rows, np.int8)
    cnt, info, cwa, met = sentinel_outputs(len(rows), d.L, d.K, d.N)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = load().lib().bchk_polar_decode_q8_host(d.handle, p(rows), len(rows), p(info), p(cwa) if cw else None, p(met),
                                                p(cnt))
    assert rc == 0, load().lib().bchk_last_error().decode()
    return cnt, info, cwa, met


def decode_q8_device(d, rows, cw=True):
    """bchk_polar_decode_q8_device into guarded, sentinel-filled device buffers; the guards are
    checked here, the rows by the caller (assert_strict)."""
    import torch
    rows = np.ascontiguousarray(rows, np.int8)
    B = len(rows)
    t_rows = torch.from_numpy(rows).to("cuda:0")
    g_info, g_cw = Guarded(B * d.L * d.K), Guarded(B * d.L * d.N)
    g_met, g_cnt = Guarded(4 * B * d.L), Guarded(4 * B)
    torch.cuda.synchronize()
    d.decode_device(t_rows.data_ptr(), B, g_info.ptr, g_cw.ptr if cw else None, g_met.ptr, g_cnt.ptr)
    d.sync()
    cnt = g_cnt.read(np.int32, (B,), "count")
    assert ((cnt >= 1) & (cnt <= d.L)).all(), cnt
    return (cnt, g_info.read(np.uint8, (B, d.L, d.K), "info"), g_cw.read(np.uint8, (B, d.L, d.N), "cw"),
            g_met.read(np.float32, (B, d.L), "metric"))


ENTRIES = (("host", decode_q8_host), ("device", decode_q8_device))

_want = {}


def expected(key, spec, rows, L):
    """(the restatement's lists of the rows, the share of its g steps that clamp): computed once
    per (key, L), shared, unchanged."""
    if (key, L) not in _want:
        sclist_q8.STATS.update(g=0, clamped=0)
        want = restated(spec, rows, L)
        _want[key, L] = rows.copy(), want, sclist_q8.STATS["clamped"] / max(sclist_q8.STATS["g"], 1)
    kept, want, share = _want[key, L]
    np.testing.assert_array_equal(kept, rows)
    return want, share


def uniform_rows(B, N, seed):
    """Uniform int8 rows, -128 (read as -127) included; row 0 is all zero."""
    rows = np.random.default_rng(seed).integers(-128, 128, (B, N)).astype(np.int8)
    rows[0] = 0
    rows[1, :2] = -128, 127
    return rows


# ================================================================ CPU: the restatement

DENSE_CPU = ["dyn_arikan_n8_a64", "dyn_arikan_n7_a33"]
DENSE_CPU_SEED = 1


@functools.lru_cache(maxsize=None)
def unit_rows(name):
    """12 rows over {-1, 0, 1}: row 0 all zero, row 1 with every second LLR zero."""
    U = 1 << dense_codes.ARIKAN[name]["n"]
    rows = np.random.default_rng(DENSE_CPU_SEED).integers(-1, 2, (12, U)).astype(np.int8)
    rows[0] = 0
    rows[1, ::2] = 0
    return rows


@pytest.mark.parametrize("L", [1, 4, 8, 32])
@pytest.mark.parametrize("name", DENSE_CPU)
def test_q8_restatement_equals_the_oracle_on_dense_constraints(name, L):
    """33 and 64 constraints live at once. With LLRs in {-1, 0, 1} the recursion stays in small
    integers, exact in f32, as long as no g step clamps -- which the data decides at U > 127 and
    this test asserts over all rows -- so the restatement and the C oracle must give the same
    lists, metrics included."""
    spec, rows = dense_codes.spec(name), unit_rows(name)
    assert rows.shape[1] == header(spec)[0] and set(np.unique(rows)) == {-1, 0, 1}
    assert not rows[0].any() and not rows[1, ::2].any() and rows[1, 1::2].any()
    sclist_q8.STATS.update(g=0, clamped=0)
    got = restated(spec, rows, L)
    assert sclist_q8.STATS["g"] > 0 and sclist_q8.STATS["clamped"] == 0
    assert_same(got, PolarOracle(spec).decode_batch(rows.astype(np.float32), L))


EDGES = {k: v for k, v in dict(SHORT_LISTS, **EDGE_K).items() if k.startswith("A") and "G" not in k}
EDGE_AMP = {8: 15, 16: 7, 32: 3}  # U max|llr| <= 127: no g step can clamp


def edge_rows(U, seed):
    amp = EDGE_AMP[U]
    rng = np.random.default_rng(seed)
    rows = rng.integers(-amp, amp + 1, (12, U)).astype(np.int8)
    rows[0] = 0
    rows[1, ::2] = 0
    rows[2] = amp * np.where(rng.integers(0, 2, U) != 0, 1, -1)
    assert U * int(np.abs(rows).max()) <= 127
    return rows


@pytest.mark.parametrize("name", list(EDGES))
def test_q8_restatement_equals_the_oracle_at_the_edges(name):
    """Lists shorter than L, K = 0 and K = U: the count is min(2^K, L), and the K = 0 row is the
    frozen word with the oracle's metric."""
    build, L, count = EDGES[name]
    spec = build()
    N, K = header(spec)[:2]
    assert count == min(1 << K, L)
    rows = edge_rows(N, seed=len(name) + K)
    sclist_q8.STATS.update(g=0, clamped=0)
    got = restated(spec, rows, L)
    assert sclist_q8.STATS["clamped"] == 0
    assert (got[0] == count).all() and got[1].shape == (12, L, K)
    want = PolarOracle(spec).decode_batch(rows.astype(np.float32), L)
    assert_same(got, want)
    if K == 0:
        assert not got[2][:, 0].any()  # the frozen word of a code without constraint terms: zero


def test_edges_are_the_arikan_short_lists_and_both_edge_dimensions():
    assert sorted(EDGES) == ["A3-K1-L32", "A4-K0-L4", "A4-K16-L8", "A5-K2-L8", "A5-K3-L32"]
    assert {header(EDGES[k][0]())[0] for k in EDGES} == set(EDGE_AMP)


# ================================================================ 3. lists shorter than L, guards

Q8_SHORT_LISTS = ["A3-K1-L32", "A5-K2-L8", "A5-K3-L32"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", Q8_SHORT_LISTS)
def test_gpu_q8_short_lists_leave_the_other_rows_and_the_guards(name, monkeypatch):
    """2^K < L: count = 2^K, rows past it untouched, guards intact, through both entry points, in
    every state; 70 words over 3 workgroups, which reuse their state from word to word."""
    monkeypatch.setenv("BCHK_POLAR_GRID", "3")
    build, L, count = SHORT_LISTS[name]
    spec = build()
    N, K = header(spec)[:2]
    assert (1 << K) == count < L
    rows = uniform_rows(70, N, seed=11 + K)
    want, _ = expected(name, spec, rows, L)
    assert (want[0] == count).all()
    for label, state, split in q8_states(spec):
        with q8_context(spec, L, state, split) as d:
            assert d.state_info()["grid"] == 3
            for how, fn in ENTRIES:
                got = fn(d, rows)
                assert (got[0] == count).all(), f"{name} {label} {how}"
                assert_strict(got, want, f"{name} {label} {how}")


# ================================================================ 4. cw = NULL

# name -> (layers, L): the shortened codes have N % 4 != 0 (byte stores of the codeword rows),
# NULL_CW_SPECS' Arikan codes N % 4 == 0 (packed stores)
Q8_NULL_CW_CODES = {"arikan_n6": (6, 8), "arikan_n7": (7, 4), "A7-N128": (7, 8), "A8-N256": (8, 4), "A6-N60": (6, 8)}
Q8_NULL_CW = [(state, name, split) for name, (n, _) in Q8_NULL_CW_CODES.items()
              for state, split in [("lds", None)] + [("tiered_q8", s) for s in (1, n // 2, n)]]


def null_cw_spec(name):
    return NULL_CW_SPECS[name]() if name in NULL_CW_SPECS else short_spec(name)


def test_q8_cw_null_cases_cover_both_store_shapes(kdir):
    for state in ("lds", "tiered_q8"):
        names = {c[1] for c in Q8_NULL_CW if c[0] == state}
        assert any(header(null_cw_spec(n))[0] % 4 == 0 for n in names)
        assert any(header(null_cw_spec(n))[0] % 4 != 0 for n in names)
    for name, (n, _) in Q8_NULL_CW_CODES.items():
        N, _, layers = header(null_cw_spec(name))[:3]
        assert layers == n and (N % 4 == 0) == (name in NULL_CW_SPECS), name
        splits = sorted(c[2] for c in Q8_NULL_CW if c[1] == name and c[0] == "tiered_q8")
        assert splits[0] == 1 < splits[1] < splits[2] == n


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(Q8_NULL_CW_CODES))
def test_gpu_q8_cw_null(name, kdir):
    """d_cw = 0 / cw = NULL: count, info and metric as with a cw buffer (itself the restatement's),
    bit for bit, and a sentinel-filled buffer that is not passed stays as it is."""
    spec, L = null_cw_spec(name), Q8_NULL_CW_CODES[name][1]
    rows = noisy_rows(spec, 12, 2.0, seed=13 + len(name))
    want, _ = expected("null-" + name, spec, rows, L)
    for state, _, split in [c for c in Q8_NULL_CW if c[1] == name]:
        with q8_context(spec, L, state, split) as d:
            for how, fn in ENTRIES:
                what = f"{name} {state} split {split} {how}"
                full = fn(d, rows)
                assert_strict(full, want, what)
                assert_strict(fn(d, rows, cw=False), full, what + " cw = NULL", cw=False)


# ================================================================ 5. epilogue store shapes

def store_splits(n):
    return None if n < 9 else (1, n // 2, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,punct", STORES, ids=[f"A{c[0]}-K{c[1]}-N{(1 << c[0]) - len(c[2])}" for c in STORES])
@pytest.mark.parametrize("L", [1, 8])
def test_gpu_q8_epilogue_store_shapes(n, K, punct, L):
    """The packed (K % 4 == 0, N % 4 == 0) and the byte stores in all four combinations, with K past
    one 32-bit record word and, at K = 264, the packed information loop in its second lane round."""
    spec = arikan_spec(n, K, dyn=3, punct=punct, seed=n + K)
    rows = noisy_rows(spec, 8, 2.0, seed=n + K + L)
    want, share = expected(f"stores-{n}-{K}", spec, rows, L)
    print(f"stores U={1 << n} K={K} L={L}: {100 * share:.1f} % of the g steps clamp")
    for label, state, split in q8_states(spec, store_splits(n)):
        with q8_context(spec, L, state, split) as d:
            assert_strict(decode_q8_host(d, rows), want, f"stores {n} {K} {label} L={L}")


def test_q8_store_shapes_cover_what_they_name():
    shapes = {(K % 4 == 0, ((1 << n) - len(p)) % 4 == 0) for n, K, p in STORES}
    assert len(shapes) == 4
    assert any(K % 4 == 0 and K // 4 > 64 for n, K, p in STORES)  # a second round of the packed information loop
    assert any(K % 4 != 0 and K > 64 for n, K, p in STORES) and all(K > 32 for n, K, p in STORES)
    assert store_splits(9) == (1, 4, 9) and all(store_splits(n) is None for n, _, _ in STORES if n < 9)


# ================================================================ 6. K = 0 and K = U

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE_K))
def test_gpu_q8_dimension_zero_and_nothing_frozen(name):
    """K = 0: one row, the frozen word, with the restatement's metric, and no information byte
    written; K = U at L = 8. Every state, both entry points, saturating rows."""
    build, L, count = EDGE_K[name]
    spec = build()
    N, K = header(spec)[:2]
    rows = uniform_rows(12, N, seed=K + 2)
    want, _ = expected(name, spec, rows, L)
    assert (want[0] == count).all()
    for label, state, split in q8_states(spec):
        with q8_context(spec, L, state, split) as d:
            for how, fn in ENTRIES:
                assert_strict(fn(d, rows), want, f"{name} {label} {how}")


# ================================================================ 7. dense dynamic freezing

DENSE = [(name, L) for name in DENSE_CPU for L in (2, 8, 32)] + [("dyn_arikan_n9_a64", 8)]
DENSE_ROWS, DENSE_RESTATED, DENSE_SNR = 96, 16, 1.0
# noisy_rows' quantiser ranges, 127 twice: at rates 1/4 and 1 dB the LLRs are small, and with a third
# of the rows each at 31, 63 and 127 the clamping share of the (128, 32) code is 0.10 +- 0.005
# whatever the seed (the rows at 31 clamp 5 % of their g steps, those at 127 18 %); with these
# ranges it is 0.12 to 0.14 on both codes, computed by the restatement on the CPU
DENSE_QMAXES = (31, 63, 127, 127)


def is_codeword_list(name, got, what):
    cnt, info, cw, _ = got
    keep = np.arange(info.shape[1])[None, :] < cnt[:, None]
    np.testing.assert_array_equal(direct_encode(name, info[keep]), cw[keep], err_msg=f"{what}: a list entry is no codeword")


@pytest.mark.gpu
@pytest.mark.parametrize("name,L", DENSE, ids=[f"{c[0]}-L{c[1]}" for c in DENSE])
def test_gpu_q8_dense_dynamic_freezing(name, L):
    """33 and 64 constraints live at once, constraints of 65 and 130 terms (n = 9): the LDS state's
    first 16 rows against the restatement, with a sizeable share of the g steps clamping; 96 rows
    in the tiered state at every split against the LDS state; every entry returned a codeword."""
    spec = dense_codes.spec(name)
    rows = noisy_rows(spec, DENSE_ROWS, DENSE_SNR, seed=len(name) + L, qmaxes=DENSE_QMAXES)
    want, share = expected(name, spec, rows[:DENSE_RESTATED], L)
    print(f"{name} L={L}: {100 * share:.1f} % of the g steps clamp")
    assert share > 0.10
    with q8_context(spec, L) as d:
        lds = decode_q8_host(d, rows)
    assert_strict(tuple(a[:DENSE_RESTATED] for a in lds), want, f"{name} q8-lds L={L}")
    assert_strict(lds, lds, f"{name} q8-lds L={L}")  # the rows past each count
    is_codeword_list(name, lds, f"{name} q8-lds L={L}")
    for label, state, split in q8_states(spec)[1:]:
        with q8_context(spec, L, state, split) as d:
            got = decode_q8_host(d, rows)
        assert_strict(got, lds, f"{name} {label} L={L}")
        is_codeword_list(name, got, f"{name} {label} L={L}")


# ================================================================ 8. genie on int8 contexts

GENIE = {"A7": lambda: arikan_spec(7, 64, dyn=4, seed=3), "arikan_n6": lambda: short_spec("arikan_n6")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GENIE))
def test_gpu_q8_genie_on_int8_contexts(name, kdir):
    """"An int8 context takes every other bchk_polar_* call" (include/bchk.h): genie_device's
    decision LLRs, u rows and counters and genie_run's totals on an int8 LDS context and on tiered
    ones at split 1 and n are those of an f32 LDS-state context. Then genie calls and int8 decodes
    interleaved on the int8 context, which share its LLR buffer (bytes in one, floats in the other)."""
    import torch
    from test_polar_contract import _genie, _same_bits, context
    spec = GENIE[name]()
    B, L = 48, 4
    with context(spec, L) as d:
        t_info = torch.zeros((B, d.K), dtype=torch.uint8, device="cuda:0")
        t_llr = torch.zeros((B, d.N), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        d.generate_device(2.0, B, t_llr.data_ptr(), t_info.data_ptr(), seed=5)
        d.sync()
        want = _genie(d, t_info, t_llr, B)
        want_run = d.genie_run(2.0, 100, seed=5, batch=37)[:2]
        llr = t_llr.cpu().numpy()
    assert want[0].sum() > 0  # decision errors occurred
    rows = load().quantize(llr[:16], 63 / 6.0, 63)
    want_lists, _ = expected("genie-" + name, spec, rows, L)
    n = header(spec)[2]
    for label, state, split in q8_states(spec, (1, n)):
        with q8_context(spec, L, state, split) as d:
            _same_bits(_genie(d, t_info, t_llr, B), want, label)
            _same_bits(d.genie_run(2.0, 100, seed=5, batch=37)[:2], want_run, label)
            assert_strict(decode_q8_host(d, rows), want_lists, label)
            _same_bits(d.genie_run(2.0, 100, seed=5, batch=37)[:2], want_run, label)
            assert_strict(decode_q8_device(d, rows), want_lists, label)
            _same_bits(_genie(d, t_info, t_llr, B), want, label)
