"""Time-budgeted SC-list decoding (polar_mixed.hip suspend / resume, polar_host.cpp's launch
loop) at EVERY suspension point.

A code with a search layer is decoded by a series of launches: past the budget a wave saves
its codeword's whole list state (a header, six registers per lane, two LDS regions, and inside
a search its scratch and the live part of its stack) and the next launch restores it. Where a
wave stops depends on the clock, so a budget of milliseconds samples a few suspension points.
A budget of one tick of the 100 MHz clock (TINY) removes the clock from the picture: the
kernel starts or resumes a wave's first unfinished codeword whatever the clock says and a search
runs at least one round per launch, so every wave does exactly one search round per launch
(one search item with BCHK_POLAR_NO_MID) and suspends -- every round of every item of every
phase is a suspension point, deterministically.

References: the C restatement (PolarOracle; for kernels up to 32 its LLRs come from
enumeration / the trellis, not from a search) and a context with the budget off (one launch).
Everything is compared bit for bit (lists, codewords, f32 metrics as uint32, counts).

What fails when `suspend` / the resume block drops a saved field (by reading polar_mixed.hip;
"forced" = test_gpu_tiny_budget_forced_search_matches_oracle, "64" = test_gpu_tiny_budget_64x64_
matches_oracle, "rounds" / "items" their two modes):

  hd[0] phase             every tiny-budget case (decoding restarts at phase 0)
  hd[1] layer rj          forced A-k16 / bch8-A-A / bch32f-A, 64 A-bch64f / bch64f-A: layers before rj
                          run again and the offset state is XORed twice
  hd[2] item rit          forced rounds at L = 4, 8: item 0 continues item rit's saved search
                          (items mode: item 0 is redone for ever -- the call does not return)
  hd[3] k                 every case (information bits land in the wrong record positions)
  hd[4] active            every L >= 2 case
  hd[5] st.top, rg[5] st.slot   L = 4, 8 at 0 / 1 dB, where full lists kill and clone paths after a resume
  hd[6] mid flag          read as 0: a search restarts at every resume, same values, and at the
                          tiny budget never ends (no assertion: the rounds cases do not return);
                          read as 1: items cases continue a stale scratch
  hd[7] sp, hd[8..9] best0 / best1, the scratch (kMlHeadBytes + 12 sp bytes: G, U, cost, |y|,
                          stack[0, sp))    forced rounds and 64 rounds: every search of 2+ rounds
  hd[10..11] hard decisions   forced rounds (low word); the high word and the sign-extension trap
                          of the low word only 64 rounds (for l <= 32 ml_metric masks bits >= l)
  hd[12..13] lrb          read as 0 it only weakens the pruning (same LLRs, more rounds): no result
                          can tell. Wrong extra bits (the sign-extension trap) over-prune: 64 rounds
  hd[14] rounds           test_gpu_round_guard_counts_rounds_across_resumes[rounds]
  rg[0] R                 every case (metrics)
  rg[1] lv                dead state: every active lane reloads lv after the layer loop, before
                          its first use -- nothing can fail
  rg[2] dm (low word)     every code with dynamic frozen symbols (all but bch64f-32)
  rg[3] dm (high word)    tests/test_polar_dense_dyn.py::test_gpu_dense_tiny_budget_matches_oracle: 34 constraints
                          live at once (mask bits 32 and 33 in use), L = 4, 8, both modes
  rg[4] rw                every case suspended with information bits pending in the record word
  LDS [0, o_ph)           every case (channel, S, C, O)
  LDS [o_act, o_tm)       act is rebuilt by list_act(active) on resume; rec: 64 bch64f-40 / A-bch64f-64 /
                          bch64f-A-60 (K > 32: a record word completed before a suspension)
  one slot per workgroup  test_gpu_budget_batch_larger_than_grid_64x64, test_gpu_tiny_budget_one_wave_
                          five_codewords, test_gpu_save_area_is_per_workgroup, test_gpu_budgeted_context_
                          reused_across_calls
"""
import ctypes as C

import numpy as np
import pytest

from bchk_pkg import load
from polar_lib import PolarOracle, awgn_llr
from test_polar_mixed import KERNELS, _same, kdir, mixed_spec  # noqa: F401
from test_polar_ml import CODES64, FORCED

pytestmark = pytest.mark.gpu

TINY = "0.00001"  # ms: one tick of the 100 MHz clock (budget_ticks = ms * 1e5)
ENV = ("BCHK_POLAR_BUDGET_MS", "BCHK_POLAR_ML", "BCHK_POLAR_GRID", "BCHK_POLAR_ML_ROUNDS")


def _decoder(mp, spec, L, kdir, budget, ml=None, grid=None, rounds=None):
    """A context with the create-time knobs set (the others cleared)."""
    for name, v in zip(ENV, (budget, ml, grid, rounds)):
        if v is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(v))
    return load().PolarListDecoder(spec, L, kernel_dir=kdir)


def _decode(mp, d, llr, no_mid=False):
    """BCHK_POLAR_NO_MID is read per call: suspend between search items only."""
    if no_mid:
        mp.setenv("BCHK_POLAR_NO_MID", "1")
    else:
        mp.delenv("BCHK_POLAR_NO_MID", raising=False)
    return d.decode(llr)


def _workload(o, K, B, snr, seed):
    info = np.random.default_rng(seed).integers(0, 2, (B, K)).astype(np.uint8)
    return awgn_llr(o.encode(info), snr, K / o.N, seed=seed + 1)


def _ids(codes):
    return ["-".join(c[0]) + f"-{c[1]}" for c in codes]


# ---- (a) every suspension point, cheap searches, an independent reference
@pytest.mark.parametrize("layers,K,dyn,punct", FORCED, ids=_ids(FORCED))
@pytest.mark.parametrize("L", [1, 4, 8])
def test_gpu_tiny_budget_forced_search_matches_oracle(kdir, layers, K, dyn, punct, L, monkeypatch):
    # BCHK_POLAR_ML=2: every matrix layer through the search, so these codes take the budgeted
    # path (any_ml follows the forced setting, polar_host.cpp); the oracle's LLRs for these
    # kernels come from enumeration / the trellis
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 17 + K)
    o = PolarOracle(spec, kdir)
    one = _decoder(monkeypatch, spec, L, kdir, "0", ml=2)
    tiny = _decoder(monkeypatch, spec, L, kdir, TINY, ml=2)
    try:
        for snr in (0.0, 2.0):
            llr = _workload(o, K, 16, snr, seed=int(snr * 10) + 3 * L + K)
            want = o.decode_batch(llr, L)
            a = _decode(monkeypatch, one, llr)
            assert one.last_launches() == 1
            _same(a, want)
            for no_mid in (False, True):
                b = _decode(monkeypatch, tiny, llr, no_mid)
                n = tiny.last_launches()
                print(f"\n{'-'.join(layers)} L={L} {snr} dB {'items' if no_mid else 'rounds'}: {n} launches")
                assert n > 1
                _same(b, want)
                _same(b, a)
    finally:
        one.close()
        tiny.close()


# ---- (b) every suspension point of the real 64 x 64 search
# The launch count of a tiny-budget call is the longest wave's round count (item count with
# NO_MID), at some tens of microseconds per launch. Per (code, L): mode -> (B, SNRs), sized
# from the measured launch counts so that a case stays within a few seconds; every (code, L)
# keeps at least one mode.
#
# Measured on an MI355X (about 40 us per launch; a rounds-mode call costs about 14 times the
# one-launch call): launches per call at B = 4, 3 dB / 1 dB unless noted --
#   rounds, L = 1: bch64f-32 26 255 / 45 895, bch64f-40 63 195 / 22 473, bch64-24 22 153 / 18 378,
#     A-bch64f-64 144 156 (B = 2, 3 dB), bch64f-A-60 76 119 (3 dB; 1 dB: 102 091 at B = 2);
#   rounds, L = 4: bch64f-40 111 908 (B = 2, 3 dB); L = 8: bch64-24 141 079 (B = 2, 3 dB); the
#     other (code, L) at L = 4, 8 take 200 000 to 1 500 000 rounds (8 to 60 s): items mode only;
#   items (the same at both SNRs and for B = 1, 2, 4): L = 1: 64 64 64 128 128, L = 4: 158 189
#     143 322 310, L = 8: 274 349 243 574 534 launches, each as long as its longest item; there
#     the cost is the decode itself and the oracle's (A-bch64f-64 at 3 dB: 1.5 s for a one-launch
#     decode of its first two codewords at L = 4, 2.8 s at L = 8 -- hence B = 2 and B = 1).
MID, ITEMS = "rounds", "items"
BOTH, HIGH = (1.0, 3.0), (3.0,)
PLAN64 = {  # (index into CODES64, L) -> {mode: (B, SNRs)}
    (0, 1): {MID: (4, BOTH), ITEMS: (4, BOTH)},
    (1, 1): {MID: (4, BOTH), ITEMS: (4, BOTH)},
    (2, 1): {MID: (4, BOTH), ITEMS: (4, BOTH)},
    (3, 1): {MID: (2, HIGH), ITEMS: (4, BOTH)},
    (4, 1): {MID: (4, HIGH), ITEMS: (4, BOTH)},
    (0, 4): {ITEMS: (4, BOTH)},
    (1, 4): {MID: (2, HIGH), ITEMS: (4, BOTH)},
    (2, 4): {ITEMS: (4, BOTH)},
    (3, 4): {ITEMS: (2, HIGH)},
    (4, 4): {ITEMS: (4, BOTH)},
    (0, 8): {ITEMS: (4, HIGH)},
    (1, 8): {ITEMS: (4, BOTH)},
    (2, 8): {MID: (2, HIGH), ITEMS: (4, BOTH)},
    (3, 8): {ITEMS: (1, HIGH)},
    (4, 8): {ITEMS: (4, HIGH)},
}
CASES64 = [(ci, L, mode) for (ci, L), modes in sorted(PLAN64.items()) for mode in sorted(modes)]


def test_plan_keeps_every_code_and_list_size():
    assert {k for k, v in PLAN64.items() if v} == {(ci, L) for ci in range(len(CODES64)) for L in (1, 4, 8)}


@pytest.mark.parametrize("ci,L,mode", CASES64, ids=[f"{_ids(CODES64)[ci]}-L{L}-{mode}" for ci, L, mode in CASES64])
def test_gpu_tiny_budget_64x64_matches_oracle(kdir, ci, L, mode, monkeypatch):
    layers, K, dyn, punct = CODES64[ci]
    B, snrs = PLAN64[(ci, L)][mode]
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 19 + K)
    o = PolarOracle(spec, kdir)
    one = _decoder(monkeypatch, spec, L, kdir, "0")
    tiny = _decoder(monkeypatch, spec, L, kdir, TINY)
    try:
        for snr in snrs:
            llr = _workload(o, K, B, snr, seed=int(snr * 10) + 5 * L + K)
            a = _decode(monkeypatch, one, llr)
            b = _decode(monkeypatch, tiny, llr, no_mid=(mode == ITEMS))
            n = tiny.last_launches()
            print(f"\n{_ids(CODES64)[ci]} L={L} B={B} {snr} dB {mode}: {n} launches")
            assert n > 1
            _same(b, a)
            _same(b, o.decode_batch(llr, L))
    finally:
        one.close()
        tiny.close()


# ---- (c) a batch larger than the grid: a wave's stride loop meets finished, suspended and
# untouched codewords in one launch, over many launches, and reuses its one save slot
_GRID3 = {}  # the batch and its two references, computed once for both budgets


def _grid3_reference(kdir, mp):
    if not _GRID3:
        layers, K, dyn, punct = CODES64[0]
        spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 19 + K)
        o = PolarOracle(spec, kdir)
        llr = _workload(o, K, 20, 3.0, seed=71)
        one = _decoder(mp, spec, 4, kdir, "0")  # one launch, a wave per codeword
        try:
            a = _decode(mp, one, llr)
        finally:
            one.close()
        rows = np.array([0, 2, 5, 7, 10, 13, 16, 19])  # the oracle on 8 rows, the one-launch lists on all 20
        _GRID3.update(spec=spec, llr=llr, one=a, rows=rows, oracle=o.decode_batch(llr[rows], 4))
    return _GRID3


# (tiny budget: between items -- 20 codewords' rounds through three waves would be some
# 10^6 launches; the 1 ms budget suspends inside the searches)
@pytest.mark.parametrize("budget,no_mid", [(TINY, True), ("1", False)], ids=["tiny-items", "1ms"])
def test_gpu_budget_batch_larger_than_grid_64x64(kdir, budget, no_mid, monkeypatch):
    ref = _grid3_reference(kdir, monkeypatch)
    many = _decoder(monkeypatch, ref["spec"], 4, kdir, budget, grid=3)
    try:
        b = _decode(monkeypatch, many, ref["llr"], no_mid)
        print(f"\ngrid 3, B = 20, budget {budget} ms: {many.last_launches()} launches")
        assert many.last_launches() > 1
        _same(b, ref["one"])
        _same(tuple(x[ref["rows"]] for x in b), ref["oracle"])
    finally:
        many.close()


@pytest.mark.parametrize("no_mid", [False, True], ids=[MID, ITEMS])
def test_gpu_tiny_budget_one_wave_five_codewords(kdir, no_mid, monkeypatch):
    layers, K, dyn, punct = FORCED[0]
    L, B = 4, 5
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 17 + K)
    o = PolarOracle(spec, kdir)
    llr = _workload(o, K, B, 1.0, seed=73)
    tiny = _decoder(monkeypatch, spec, L, kdir, TINY, ml=2, grid=1)
    try:
        b = _decode(monkeypatch, tiny, llr, no_mid)
        assert tiny.last_launches() > B
        _same(b, o.decode_batch(llr, L))
    finally:
        tiny.close()


# ---- (d) nothing leaks between calls on one context; rows past count keep the caller's fill
def _decode_filled(d, llr):
    """bchk_polar_decode_host on caller-filled outputs."""
    B = llr.shape[0]
    info = np.full((B, d.L, d.K), 0xAB, np.uint8)
    cw = np.full((B, d.L, d.N), 0xCD, np.uint8)
    met = np.full((B, d.L), -12345.5, np.float32)
    cnt = np.full(B, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = load().lib().bchk_polar_decode_host(d.handle, p(llr), B, p(info), p(cw), p(met), p(cnt))
    assert rc == 0
    return cnt, info, cw, met


def test_gpu_budgeted_context_reused_across_calls(kdir, monkeypatch):
    # K = 3 under L = 16: 8 paths at most, so every codeword leaves list rows unwritten
    layers, K, L = ("bch16", "A"), 3, 16
    spec = mixed_spec(layers, K, 0, (), seed=5)
    o = PolarOracle(spec, kdir)
    tiny = _decoder(monkeypatch, spec, L, kdir, TINY, ml=2)
    try:
        for call, (B, no_mid) in enumerate([(12, False), (5, True), (12, False)]):
            llr = _workload(o, K, B, 0.0, seed=80 + call)
            fresh = _decoder(monkeypatch, spec, L, kdir, "0", ml=2)
            try:
                a = fresh.decode(llr)
            finally:
                fresh.close()
            if no_mid:
                monkeypatch.setenv("BCHK_POLAR_NO_MID", "1")
            else:
                monkeypatch.delenv("BCHK_POLAR_NO_MID", raising=False)
            cnt, info, cw, met = _decode_filled(tiny, llr)
            assert tiny.last_launches() > 1
            _same((cnt, info, cw, met), a)
            _same((cnt, info, cw, met), o.decode_batch(llr, L))
            assert (cnt < L).all() and (cnt >= 1).all()
            for b in range(B):
                assert (info[b, cnt[b]:] == 0xAB).all() and (cw[b, cnt[b]:] == 0xCD).all()
                assert (met[b, cnt[b]:] == np.float32(-12345.5)).all()
    finally:
        tiny.close()


# ---- (e) the device entry point under a budget
def test_gpu_budgeted_device_entry_point(kdir, monkeypatch):
    import torch
    layers, K, dyn, punct = CODES64[0]
    L, B = 4, 8
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 19 + K)
    o = PolarOracle(spec, kdir)
    llr = _workload(o, K, B, 2.0, seed=91)
    d = _decoder(monkeypatch, spec, L, kdir, "1")
    try:
        want = _decode(monkeypatch, d, llr)
        dev = torch.device("cuda:0")
        t_llr = torch.from_numpy(llr).to(dev)
        t_info = torch.zeros((B, L, K), dtype=torch.uint8, device=dev)
        t_cw = torch.zeros((B, L, o.N), dtype=torch.uint8, device=dev)
        t_met = torch.zeros((B, L), dtype=torch.float32, device=dev)
        t_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d.decode_device(t_llr.data_ptr(), B, t_info.data_ptr(), t_cw.data_ptr(), t_met.data_ptr(),
                        t_cnt.data_ptr())
        d.sync()
        print(f"\ndevice entry point, 1 ms: {d.last_launches()} launches")
        assert d.last_launches() > 1
        _same((t_cnt.cpu().numpy(), t_info.cpu().numpy(), t_cw.cpu().numpy(), t_met.cpu().numpy()), want)
    finally:
        d.close()


# ---- (f) the search's round guard counts the whole search, over every launch it took
@pytest.mark.parametrize("no_mid", [False, True], ids=[MID, ITEMS])
def test_gpu_round_guard_counts_rounds_across_resumes(kdir, no_mid, monkeypatch):
    # guard 8: a search still running after 8 rounds gives a NaN LLR. At the tiny budget those
    # 8 rounds are 8 launches; a guard restarted by every launch would never fire. One-launch
    # context only (the oracle has no guard); metrics (NaN included) as uint32.
    layers, K, dyn, punct = FORCED[3]
    L, B = 4, 16
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 17 + K)
    o = PolarOracle(spec, kdir)
    llr = _workload(o, K, B, 0.0, seed=97)
    one = _decoder(monkeypatch, spec, L, kdir, "0", ml=2, rounds=8)
    tiny = _decoder(monkeypatch, spec, L, kdir, TINY, ml=2, rounds=8)
    full = _decoder(monkeypatch, spec, L, kdir, "0", ml=2)
    try:
        a = _decode(monkeypatch, one, llr)
        b = _decode(monkeypatch, tiny, llr, no_mid)
        assert tiny.last_launches() > 1
        _same(b, a)
        c = _decode(monkeypatch, full, llr)
        _same(c, o.decode_batch(llr, L))
        # some search did hit the guard: the lists differ from the unguarded ones
        assert not (np.array_equal(a[1], c[1]) and np.array_equal(a[3].view(np.uint32), c[3].view(np.uint32)))
    finally:
        one.close()
        tiny.close()
        full.close()


# ---- save-area size: one slot per workgroup, 4 bytes per codeword
def test_gpu_save_area_is_per_workgroup(kdir, monkeypatch):
    layers, K, dyn, punct = FORCED[0]
    L, B, grid = 4, 4096, 8
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 17 + K)
    o = PolarOracle(spec, kdir)
    llr = _workload(o, K, B, 1.0, seed=101)
    one = _decoder(monkeypatch, spec, L, kdir, "0", ml=2, grid=grid)
    # 0.2 ms launches: each wave suspends somewhere in its 512 codewords, launch after launch
    many = _decoder(monkeypatch, spec, L, kdir, "0.2", ml=2, grid=grid)
    try:
        a = _decode(monkeypatch, one, llr)
        assert one.scratch_bytes()[0] == 0  # budget off: no scratch at all
        b = _decode(monkeypatch, many, llr)
        print(f"\nB = {B}, grid {grid}, 0.2 ms: {many.last_launches()} launches")
        assert many.last_launches() > 1
        _same(b, a)
        rows = np.arange(0, B, 64)
        _same(tuple(x[rows] for x in b), o.decode_batch(llr[rows], L))
        scratch, stride = many.scratch_bytes()
        print(f"scratch {scratch} B, save slot {stride} B")
        assert 0 < stride <= 64 + 64 * 24 + 160 * 1024 + 16 * 1024  # header, registers, LDS, search scratch
        assert scratch <= grid * stride + 4 * B + 8
    finally:
        one.close()
        many.close()
