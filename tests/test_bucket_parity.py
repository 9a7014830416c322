"""GPU parity at every kernel bucket: each (M, TMAX) kernel set of select_kernels, and each
combination of stages a code can have (fast / first kernel, lane pre-pass, selection first
kernel, syndrome table, analytic tail: bchk_kernel_info), against the reference's recorded
vectors and the C oracle. Bit-exact on words, path metrics (f64 bits), counters and flags.

CASES is the one table of codes; tests/test_abi.py's completeness test reads it and fails
when a dispatch group has no case."""
import os

import numpy as np
import pytest

from bchk_pkg import load
from golden import load_vectors, vector_j15_files
from oracle_lib import Oracle
from test_gpu_parity import PATHS, check_against

# (m, t, J, Eb/N0 dB, seed): per dispatch group (bchk_kernel_info) its lowest t, its top t and,
# where it holds three or more, one t inside -- the (m, t, J) of the fixtures oracle/make_golden.py
# lists among them. J = 15 wherever the reference's uncapped loop is too long.
# The noise is the fixture's, except (8,17): 4.5 dB (at 4 dB three words in four run to the
# 2^15 - 1 bound, too many for a batch of one wave per codeword) and (7,31): 9 dB (one word at
# the bound takes the oracle seconds; fewer of them). (6,31): the fixture's noise; the batch's
# seed (6) is one whose first 512 words hold two of more than 512 decodes (one word in about
# 800 does).
CASES = [
    (2, 1, -1, 3.0, 5),
    (3, 1, -1, 3.0, 5), (3, 2, -1, 3.0, 5), (3, 3, -1, 3.0, 5),
    (4, 1, -1, 3.0, 5), (4, 2, -1, 3.0, 5), (4, 3, -1, 3.0, 5), (4, 4, -1, 3.0, 5), (4, 7, -1, 3.0, 5),
    (5, 1, -1, 4.0, 5), (5, 2, -1, 4.0, 5), (5, 3, -1, 4.0, 5), (5, 4, -1, 4.0, 5), (5, 6, -1, 4.0, 5),
    (5, 7, 15, 4.0, 5), (5, 8, 15, 4.0, 5),
    (5, 9, 15, 4.0, 5), (5, 12, 15, 4.0, 5), (5, 15, 15, -10.0, 5),
    (6, 1, 15, 5.0, 5), (6, 4, 15, 4.0, 5), (6, 6, 15, 4.0, 5), (6, 7, 15, 3.0, 5), (6, 9, 15, 5.0, 5), (6, 12, 15, 5.0, 5),
    (6, 13, 15, 5.0, 5), (6, 15, 15, 5.0, 5), (6, 31, 15, -12.0, 5),
    (7, 1, 15, 4.0, 5), (7, 4, 15, 4.0, 5), (7, 8, 15, 3.5, 5), (7, 9, 15, 3.5, 5), (7, 12, 15, 4.0, 5), (7, 16, 15, 5.5, 5),
    (7, 17, 15, 5.5, 5), (7, 24, 15, 7.0, 5), (7, 31, 15, 9.0, 5),
    (8, 1, 15, 2.0, 5), (8, 8, 15, 4.5, 5), (8, 15, 15, 5.0, 5), (8, 16, 15, 4.5, 5), (8, 17, 15, 4.5, 5), (8, 20, 15, 5.0, 5), (8, 32, 15, 7.5, 5),
]
# the top t of a group where it has no case: the reference does not finish (7,32) words, and
# neither does the oracle (oracle/make_golden.py), so t = 31 stands for the top of <7,32>
TOP_INSTEAD = {(7, 32): 31}
# codes of which the reference takes more than 2 s for 32 words at the case's noise: 67 rows
# against the oracle instead of 257
SLOW = {(8, 15), (5, 8), (5, 9), (5, 12), (6, 12), (6, 15), (7, 16), (7, 17), (7, 24), (7, 31), (8, 16), (8, 17), (8, 20),
        (8, 32)}
# (5,15), a repetition code with 2t + 1 = n: no word of 20 000 to 60 000 per noise level from
# -60 to 5 dB took more than 8 chunks of patterns (VECTORS_J15 in oracle/make_golden.py), so
# its batch is not asked to reach the cooperative kernel.
NO_HEAVY = {(5, 15)}
# (m, t, J, Eb/N0): one case per kernel set this module adds, for the edge rows; n = 3 and
# n = 7 also with J = 15 > n. <7,32> by t = 31: the oracle does not finish (7,32) rows.
EDGE = [(2, 1, -1, 3.0), (2, 1, 15, 3.0), (3, 1, 15, 3.0), (3, 3, -1, 3.0), (3, 3, 15, 3.0), (4, 7, -1, 3.0),
        (5, 8, 15, 4.0), (5, 15, 15, -10.0), (6, 12, 15, 5.0), (6, 31, 15, -12.0), (7, 16, 15, 6.0), (7, 31, 15, 9.5),
        (8, 16, 15, 5.5), (8, 32, 15, 8.0)]
TOPS = [(2, 1), (3, 3), (4, 2), (4, 7), (5, 3), (5, 8), (5, 15), (6, 6), (6, 12), (6, 31), (7, 8), (7, 16), (7, 32),
        (8, 15), (8, 16), (8, 32)]

pytestmark = pytest.mark.gpu


def _id(c):
    return "m%dt%d_J%d" % c[:3]


_live = {"key": None, "ctx": {}}


def dec(m, t, J, path="fast+exact+tail"):
    """Contexts of one (m, t, J) at a time, one per execution path (test_gpu_parity.PATHS)."""
    if _live["key"] != (m, t, J):
        for d in _live["ctx"].values():
            d.close()
        _live["key"], _live["ctx"] = (m, t, J), {}
    if path not in _live["ctx"]:
        fast, limit, filt, analytic = PATHS[path]
        old = os.environ.pop("BCHK_CHUNK_LIMIT", None)
        if limit is not None:
            os.environ["BCHK_CHUNK_LIMIT"] = limit
        try:
            d = load().KanekoKernelProcessor(m, t, J=J)
        finally:
            os.environ.pop("BCHK_CHUNK_LIMIT", None)
            if old is not None:
                os.environ["BCHK_CHUNK_LIMIT"] = old
        d.set_fast_path(fast)
        d.set_syndrome_table(filt)
        d.set_analytic(analytic)
        _live["ctx"][path] = d
    return _live["ctx"][path]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for d in _live["ctx"].values():
        d.close()
    _live["key"], _live["ctx"] = None, {}


def fill_of(B, n):
    return (np.arange(B * n, dtype=np.uint64).reshape(B, n) % 3 == 0).astype(np.uint8)


def assert_same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    rows = np.flatnonzero(a[2] != b[2])
    assert rows.size == 0, [(int(r), a[2][r], b[2][r]) for r in rows[:4]]


@pytest.mark.parametrize("exec_path", list(PATHS))
@pytest.mark.parametrize("path", vector_j15_files(), ids=os.path.basename)
def test_kaneko_j15_matches_reference_vectors(path, exec_path):
    # a path a code does not have (no table at t > 7, no tail at TMAX > 8, no fast kernel) must
    # still give the reference's result
    v = load_vectors(path)
    d = dec(v.m, v.t, 15, exec_path)
    assert (d.n, d.k) == (v.n, v.k)
    np.testing.assert_array_equal(d.g, v.g)
    res, l0, st = d.decode(v.y)
    check_against(v.res, v.l0, v.decodes, v.cmp, v.sums, v.accepted, res, l0, st)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_row_matches_oracle(case):
    # a ragged batch; with a stats record, and through the fused call without one (the
    # selection kernels, or none at TMAX = 32); rows never accepted keep the caller's bytes
    import torch
    m, t, J, snr, seed = case
    d = dec(m, t, J)
    B = 67 if (m, t) in SLOW else 257
    n = d.n
    tx, y, _ = d.generate(snr, B, seed=seed)
    fill = fill_of(B, n)
    res, l0, st = d.decode(y, res=fill.copy())
    r2, l2, s2, a2 = Oracle(m, t).kaneko_batch(y, J=J)
    check_against(r2, l2, s2[:, 0], s2[:, 1], s2[:, 2], a2, res, l0, st)
    acc = a2.astype(bool)
    np.testing.assert_array_equal(res[~acc], fill[~acc])
    dy, dtx = torch.from_numpy(y).cuda(), torch.from_numpy(tx).cuda()
    dres = torch.from_numpy(fill.copy()).cuda()
    dl0 = torch.zeros(B, dtype=torch.float64, device="cuda")
    c6 = torch.tensor([3, 5, 7, 11, 13, 17], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d.decode_count_device(dy.data_ptr(), dtx.data_ptr(), B, dres.data_ptr(), dl0.data_ptr(), 0, c6.data_ptr())
    d.sync()
    r1 = dres.cpu().numpy()
    np.testing.assert_array_equal(r1[acc], r2[acc])
    np.testing.assert_array_equal(r1[~acc], fill[~acc])
    np.testing.assert_array_equal(dl0.cpu().numpy()[acc].view(np.uint64), l2[acc].view(np.uint64))
    err = (r1 != tx).sum(axis=1)
    want = [3 + int((err > 0).sum()), 5 + int(err.sum()), 7 + int(s2[:, 0].sum()), 11 + int(s2[:, 1].sum()),
            13 + int(s2[:, 2].sum()), 17 + B]
    np.testing.assert_array_equal(c6.cpu().numpy(), want)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_default_path_equals_exact_only_at_batch(case):
    F = load()
    m, t, J, snr, seed = case
    d, ex = dec(m, t, J), dec(m, t, J, "exact-only")
    B = 4096
    _, y, _ = d.generate(snr, B, seed=seed + 1)
    cap = (1 << 24) if J < 0 else 0  # as test_small_code_uncapped_tail_lists_codewords
    d.set_max_decodes(cap)
    ex.set_max_decodes(cap)
    a = d.decode(y)
    to_exact, to_coop = d.path_counts()
    to_tail, coop = d.tail_count(), d.coop_stats()
    b = ex.decode(y)
    d.set_max_decodes(0)
    ex.set_max_decodes(0)
    assert_same(a, b)
    assert not np.any(a[2]["flags"] & F.F_TRUNCATED)
    info = F.kernel_info(m, t)
    heavy = int((a[2]["decodes"] > 8 * 64).sum())
    print(f"\nstages {_id(case)} {snr:g} dB: {info} first-pass queue {to_exact} tail {to_tail} coop {to_coop} "
          f"coop_stats {coop} rows > 512 decodes {heavy} max {int(a[2]['decodes'].max())}")
    if J == 15 and info["tmax"] > 8 and (m, t) not in NO_HEAVY:
        assert to_coop > 0 and heavy > 0
    if info["tail"] and heavy:
        assert to_tail > 0


@pytest.mark.parametrize("m,t,J,snr", EDGE, ids=lambda v: str(v))
def test_edge_rows(m, t, J, snr):
    # exact |y| tie, 1-ulp prefix tie (long codes), 0.0, 1e-300, 1e300, a noiseless codeword:
    # tied rows flagged, every other row equal to the oracle
    F = load()
    o = Oracle(m, t)
    n = o.n
    d = dec(m, t, J)
    tx, y, _ = d.generate(snr, 16, seed=303)
    y = y.copy()
    y[0, 0] = -y[0, n - 1]
    if m >= 7:
        y[1, 3] = np.nextafter(y[1, 8], np.inf if y[1, 8] > 0 else -np.inf)
        y[6, n - 1] = -y[6, 0] * (1 + 2.0 ** -50)
    y[2, 1] = 1e-300
    y[3, 1] = 1e300
    y[4, n // 2] = 0.0
    y[5, :] = np.where(tx[5] == 1, 1.0, -1.0)
    plain = np.setdiff1d(np.arange(len(y)), [0, 5])
    r2, l2, s2, a2 = o.kaneko_batch(y[plain], J=J)
    acc = a2.astype(bool)
    for path in ("fast+exact+tail", "exact-only", "coop-heavy"):
        dd = dec(m, t, J, path)
        dd.set_max_decodes(1 << 16)
        fill = fill_of(len(y), n)
        res, l0, st = dd.decode(y, res=fill.copy())
        dd.set_max_decodes(0)
        assert st["flags"][0] & F.F_TIE and st["flags"][5] & F.F_TIE, path  # (plain rows: check_against)
        check_against(r2, l2, s2[:, 0], s2[:, 1], s2[:, 2], a2, res[plain], l0[plain], st[plain])
        np.testing.assert_array_equal(res[plain][~acc], fill[plain][~acc])


@pytest.mark.parametrize("m,t", TOPS, ids=lambda v: str(v))
def test_alg_decoder_from_syndromes_matches_oracle(m, t):
    # Decoder::decode from explicit syndromes S_1, S_3, .. S_{2t-1} on error patterns of weight
    # 0 .. t + 3 (the zero codeword sent), against the oracle's Euclid decoder on the words
    o = Oracle(m, t)
    n = o.n
    rng = np.random.default_rng(100 * m + t)
    alog = np.array(o.code.alog[:n], np.uint32)
    odd = 2 * np.arange(t) + 1
    N = 2000
    words = np.zeros((N, n), np.uint8)
    S = np.zeros((N, t), np.uint32)
    for b in range(N):
        pos = rng.choice(n, size=min(n, int(rng.integers(0, t + 4))), replace=False)
        words[b, pos] = 1
        if len(pos):
            S[b] = np.bitwise_xor.reduce(alog[np.outer(pos, odd) % n], axis=0)
    ok, flips = dec(m, t, -1).alg_decode(np.zeros_like(words), syndromes=S)
    want = [o.alg_decode(w, bm=False) for w in words]
    np.testing.assert_array_equal(ok, [w[0] for w in want])
    ans = np.array([w[1] for w in want])
    np.testing.assert_array_equal(flips[ok], (ans ^ words)[ok])
    assert ok.sum() > N // 4
