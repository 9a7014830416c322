"""The six SC-list kernels at list sizes that are no power of two. bchk_polar_create* takes every
L from 1 to 32, and everything the kernels share is indexed by L -- plist::unfrozen_select's cut at
min(2 nact, L), the path stack with its lazy slot at lane L, the tiered kernels' ~used & lmask
search for a free array, every LDS and workspace stride, the epilogues' rows cw L + r -- while the
rest of the suite decodes at L in {1, 2, 4, 8, 16, 32} only. Here LISTS = (3, 5, 6, 7, 12, 24, 31),
everything bit for bit: count, information vectors, codewords, f32 metric bits (integers for int8),
list order, over the first `count` rows.

  1  CPU  the C oracle against tests/sclist_plain.py, and tests/sclist_q8.py against sclist_plain
          where nothing saturates, at every L of LISTS; the workloads the GPU tests decode reach the
          code they are for (test_gpu_workloads_reach_the_cut: full lists, unequal metrics and, at
          odd L, a cut between the two candidates of one path -- computed from the references)
  2       the recorded lists of the compiled vendored library, tests/golden/polar_ref_lists_*,
          run by tests/test_polar_reference.py; here the 8 x 8 layer of lists_bch8_A through the
          GPU's trellis as well, and the files' size
  3  GPU  polar_sclist / polar_sclist_tiered against the oracle, every split; ties; state reuse;
          the tiered layouts restated; (2048, 1024) at L = 24, which only the tiered state takes
  4  GPU  polar_sclist_q8 against the restatement with saturating rows, polar_sclist_q8_tiered
          against it at every split; layers narrower than a word; the int8 sweep
  5  GPU  polar_mixed / polar_mixed_tiered at every split against the oracle (a code with a named
          layer: the LDS kernel against the tiered one, test_polar_mixed_tiered.reference); budgeted
          launches, whose save area holds L paths
  6  GPU  the output contract in every state: lists shorter than L between sentinels and guard
          bytes, cw = NULL, K = 0 and K = U, count_device, sweep_device

Nothing here was seen to fail: at these list sizes the six kernels give the references' lists.
Every helper is the one of the module that tests the same thing at a power of two.
"""
import functools
import os
import time

import numpy as np
import pytest

import polar_ref_lib as R
import sclist_plain
import sclist_q8
from bchk_pkg import load
from polar_lib import PolarOracle, arikan_spec, awgn_llr
from test_polar_budget import TINY, _decode, _decoder, _workload
from test_polar_contract import (EDGE_K, NULL_CW_SPECS, assert_strict, batches, context, decode_device, decode_host, header,  # noqa: F401
                                 kdir, kernel_dir, oracle, states)
from test_polar_mixed import mixed_spec
from test_polar_mixed_tiered import CODES as MIXED_CODES
from test_polar_mixed_tiered import NAMED, any_spec, check_every_split, reference, words
from test_polar_ml import FORCED
from test_polar_q8 import check as q8_check
from test_polar_q8 import noisy_rows, pipeline, q8_decoder, restated
from test_polar_q8 import assert_same as q8_assert_same
from test_polar_q8_contract import ENTRIES as Q8_ENTRIES
from test_polar_q8_contract import q8_context, q8_states, uniform_rows
from test_polar_q8_plain import SMALL as PLAIN_SMALL
from test_polar_q8_tiered import LDS_MAX, clamped_share, tiered_q8
from test_polar_q8_tiered import restated_layout as q8_restated_layout
from test_polar_q8_tiered import restated_split as q8_restated_split
from test_polar_sclist import CODES, assert_same, gpu_decoder, workload
from test_polar_tiered import AUTO_CHOICE, SMALL, tiered

LISTS = (3, 5, 6, 7, 12, 24, 31)


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print(f"\nwall time {request.node.name}: {time.perf_counter() - t0:.2f} s")


# ================================================================ the parameter tables
# One row per GPU case; test_every_state_meets_every_list_size reads the (state, L) pairs off them.

F32_LDS = [c + (L,) for c in CODES if c[0] <= 9 for L in LISTS] + [(10, 512, 20, (), 12)]  # U L = 12 288 fits LDS
F32_TIERED = [c + (L,) for c in SMALL for L in LISTS]
TIE_LISTS = (3, 6, 7)
REUSE_L, LAYOUT_LISTS, PAST_LDS = 7, (7, 31), (11, 1024, 24)
Q8_LDS = [(n, L) for n in (6, 7, 8) for L in LISTS]
Q8_TIERED = [c + (L,) for c in SMALL if c[0] in (5, 6, 8) for L in (3, 6, 7, 31)]
Q8_NARROW, Q8_SWEEP_L = [(2, 2, 3), (3, 4, 3)], 6
MIXED = [c + (L,) for c in MIXED_CODES for L in (3, 6, 7, 12)]
BUDGET = [FORCED[0] + (L,) for L in (3, 6)]
SHORT = [(1, 3, 2), (2, 5, 4), (2, 7, 4), (3, 12, 8), (4, 24, 16), (4, 31, 16)]  # K, L, count
NULL_L, EDGE_L, COUNT_L, SWEEP_L = 5, 3, 7, 6
F32_STATES, Q8_STATES = ("lds", "tiered", "tiered_mixed", "mixed"), ("q8", "tiered_q8")


def is_named(layers):
    return any(n in NAMED and n != "A" for n in layers)


def test_every_state_meets_every_list_size():
    """Every (state, L), the mixed LDS kernel ("mixed") among the states, in some GPU case below."""
    seen = {("lds", c[-1]) for c in F32_LDS} | {("tiered", c[-1]) for c in F32_TIERED}
    seen |= {(s, L) for s in ("lds", "tiered") for L in TIE_LISTS}
    seen |= {("q8", L) for _, L in Q8_LDS} | {("tiered_q8", c[-1]) for c in Q8_TIERED}
    seen |= {(s, c[-1]) for c in MIXED for s in ("mixed", "tiered_mixed")} | {("mixed", c[-1]) for c in BUDGET}
    seen |= {(s, L) for _, L, _ in SHORT for s in F32_STATES + Q8_STATES}
    assert seen >= {(s, L) for s in F32_STATES + Q8_STATES for L in LISTS}
    assert all(L in LISTS for _, L in seen)
    # and what the cases name: every split-dependent table holds the codes of the module it follows
    assert {c[:4] for c in F32_TIERED} == set(SMALL) and {c[:4] for c in MIXED} == set(MIXED_CODES)
    assert any(is_named(c[0]) for c in MIXED) and {c[0] for c in Q8_TIERED} == {5, 6, 8}
    assert all((1 << K) == count < L for K, L, count in SHORT)


# ================================================================ 1. CPU: the references

CPU_CODES = [(5, 16, 3), (6, 32, 4), (7, 64, 6)]  # n, K, dynamic constraints; nothing punctured
CPU_WORDS = 8


def plain_batch(spec, llr, L):
    """sclist_plain.decode over the rows, in PolarOracle.decode_batch's shapes."""
    K, U = int(spec.split()[1]), llr.shape[1]
    cnt = np.zeros(len(llr), np.int32)
    info, cw, met = np.zeros((len(llr), L, K), np.uint8), np.zeros((len(llr), L, U), np.uint8), np.zeros((len(llr), L), np.float32)
    for b, row in enumerate(llr):
        c, i, w, m = sclist_plain.decode(spec, row, L)
        cnt[b], info[b, :c], cw[b, :c], met[b, :c] = c, i, w, m
    return cnt, info, cw, met


@pytest.mark.parametrize("L", LISTS)
@pytest.mark.parametrize("n,K,dyn", CPU_CODES)
def test_oracle_equals_the_plain_decoder(n, K, dyn, L):
    """AWGN LLRs, and tie-producing ones: rounded to multiples of 4, exact zeros among them."""
    spec, o, info, llr = workload(n, K, dyn, (), 1.0 + 0.25 * n, CPU_WORDS, seed=n * 7 + L)
    ties = (4.0 * np.round(workload(n, K, dyn, (), 1.0, CPU_WORDS, seed=77 + L)[3] / 4.0)).astype(np.float32)
    assert np.all(ties % 4 == 0) and np.any(ties == 0)
    for rows in (llr, ties):
        want = plain_batch(spec, rows, L)
        assert (want[0] == L).all()
        assert_same(o.decode_batch(rows, L), want)


@pytest.mark.parametrize("L", LISTS)
@pytest.mark.parametrize("n,K,dyn,amp", PLAIN_SMALL)
def test_q8_restatement_equals_the_plain_decoder_without_saturation(n, K, dyn, amp, L):
    """test_polar_q8_plain's scheme: integer LLRs with U max|llr| <= 127, every value exact in f32."""
    U = 1 << n
    spec = arikan_spec(n, K, dyn=dyn, seed=n + dyn)
    rng = np.random.default_rng(100 * n + 10 * dyn + L)
    rows = rng.integers(-amp, amp + 1, (6, U)).astype(np.int8)
    rows[0] = 0
    rows[1, ::2] = 0
    rows[2] = amp * np.where(rng.integers(0, 2, U) != 0, 1, -1)
    assert U * int(np.abs(rows).max()) <= 127
    sclist_q8.STATS.update(g=0, clamped=0)
    got = restated(spec, rows, L)
    assert sclist_q8.STATS["g"] > 0 and sclist_q8.STATS["clamped"] == 0
    assert (got[0] == min(L, 1 << K)).all()
    q8_assert_same(got, plain_batch(spec, rows.astype(np.float32), L))


def reset_stats():
    sclist_plain.STATS.update(unfrozen=0, cut=0, three=0, split_pair=0)
    sclist_q8.STATS.update(g=0, clamped=0, split_pair=0)


def test_plain_decoder_counts_its_phases():
    """STATS on cases with a known answer: at L = 1 every unfrozen phase cuts two candidates of
    one path to one; a list as large as the code never cuts; and at L = 3 all three outcomes meet
    in one phase of some word."""
    spec, o, info, llr = workload(5, 16, 3, (), 2.25, 8, seed=1)
    reset_stats()
    sclist_plain.decode(spec, llr[0], 1)
    assert sclist_plain.STATS == dict(unfrozen=16, cut=16, three=0, split_pair=16)
    reset_stats()
    spec4 = arikan_spec(3, 4)
    assert sclist_plain.decode(spec4, workload(3, 4, 0, (), 1.0, 1, seed=2)[3][0], 16)[0] == 16
    assert sclist_plain.STATS == dict(unfrozen=4, cut=0, three=0, split_pair=0)
    reset_stats()
    for row in llr:
        sclist_plain.decode(spec, row, 3)
    s = sclist_plain.STATS
    assert s["unfrozen"] == 8 * 16 and s["cut"] == 8 * 15 and 0 < s["three"] <= s["cut"] and 0 < s["split_pair"] <= s["cut"]


# ---- the GPU workloads, computed once, shared and left unchanged

def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def f32_case(n, K, dyn, punct, L):
    """(spec, llr, the oracle's lists) of an all-Arikan case: the suite's Eb/N0 and seed rule."""
    spec, o, info, llr = workload(n, K, dyn, punct, 1.0 + 0.25 * n, 48 if n >= 10 else 96, seed=n * 7 + L)
    return (spec,) + frozen(llr) + (frozen(*o.decode_batch(llr, L)),)


@functools.lru_cache(maxsize=None)
def tie_case(L):
    spec, o, info, llr = workload(7, 64, 4, (), 1.0, 96, seed=77)
    q = np.round(llr / 4.0).astype(np.float32)
    return (spec,) + frozen(q) + (frozen(*o.decode_batch(q, L)),)


@functools.lru_cache(maxsize=None)
def reuse_case():
    spec, o, info, llr = workload(6, 32, 5, (1, 7), 2.0, 3000, seed=21)
    return (spec,) + frozen(llr) + (frozen(*o.decode_batch(llr, REUSE_L)),)


@functools.lru_cache(maxsize=None)
def q8_lds_case(n, L):
    """(spec, rows, the restatement's lists, clamped share, split-pair phases): the rows of
    test_gpu_q8_matches_restatement_with_saturation."""
    spec = arikan_spec(n, 1 << (n - 1))
    rows = noisy_rows(spec, 3, 2.0, seed=10 * n + L)
    reset_stats()
    want, share = clamped_share(spec, rows, L)
    return (spec,) + frozen(rows) + (frozen(*want), share, sclist_q8.STATS["split_pair"])


Q8_TIERED_RESTATED = 3


@functools.lru_cache(maxsize=None)
def q8_tiered_case(n, K, dyn, punct, L):
    """test_gpu_q8_tiered_every_split's rows; the restatement on the first of them."""
    spec = arikan_spec(n, K, dyn=dyn, punct=punct, seed=n * 7 + L)
    rows = noisy_rows(spec, 96, 2.0, seed=10 * n + L)
    reset_stats()
    few, share = clamped_share(spec, rows[:Q8_TIERED_RESTATED], L)
    return (spec,) + frozen(rows) + (frozen(*few), share, sclist_q8.STATS["split_pair"])


def mixed_case(layers, K, dyn, punct, L):
    """What check_every_split decodes for this case: (spec, B, Eb/N0, seed)."""
    return any_spec(layers, K, dyn, punct, seed=len(layers) * 11 + K), 96, 1.5, K + L


def budget_case(layers, K, dyn, punct, L, snr):
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 17 + K)
    o = PolarOracle(spec, kernel_dir())
    llr = _workload(o, K, 16, snr, seed=int(snr * 10) + 3 * L + K)
    return spec, o, llr


def unpunctured(spec, llr):
    """An all-Arikan specification without its punctured symbols, and the rows with the LLR 0 a
    punctured symbol is decoded with: what sclist_plain takes."""
    lines = spec.rstrip("\n").split("\n")
    N, K, _, n, nsh, npu = (int(t) for t in lines[0].split())
    assert nsh == 0
    if not npu:
        return spec, llr
    punct = [int(t) for t in lines[2].split()]
    full = np.zeros((len(llr), N + npu), np.float32)
    full[:, [i for i in range(N + npu) if i not in punct]] = llr
    return "\n".join([f"{N + npu} {K} 0 {n} 0 0", lines[1]] + lines[3:]) + "\n", full


def full_and_unequal(want, L, K, what):
    cnt, _, _, met = want
    assert (cnt == min(L, 1 << K)).any(), f"{what}: no word fills the list"
    assert any(len(set(met[b, :cnt[b]].tolist())) > 1 for b in range(len(cnt))), f"{what}: no list with two metrics"


def plain_split_pair(spec, llr, L, what):
    """Words through sclist_plain until a phase cuts between the two candidates of one path."""
    spec, llr = unpunctured(spec, llr)
    reset_stats()
    for row in llr:
        sclist_plain.decode(spec, row, L)
        if sclist_plain.STATS["split_pair"]:
            return
    raise AssertionError(f"{what}: no phase of {sclist_plain.STATS['cut']} cuts inside a pair")


def test_gpu_workloads_reach_the_cut():
    """The precondition of parts 3 to 5, from the references alone: every (code, L) decoded on the
    GPU holds a word whose list is full (count = min(L, 2^K)), a word whose list has two different
    metrics and, at odd L with 2^K > L, a phase where the cut at cand[:L] falls between the two
    candidates of one path. Split pairs are counted by the instrumented restatements, which exist
    for all-Arikan codes only (sclist_plain.STATS, sclist_q8.STATS): for a code with a matrix layer
    the first two conditions are asserted from the C oracle, and for one with a named layer, which
    has no CPU reference with a list, none. Part 6's codes are short by design:
    their condition is the count the issue names, asserted there."""
    for n, K, dyn, punct, L in sorted(set(F32_LDS + F32_TIERED)):
        spec, llr, want = f32_case(n, K, dyn, punct, L)
        what = f"f32 ({n}, {K}) L={L}"
        full_and_unequal(want, L, K, what)
        if L % 2 and (1 << K) > L:
            plain_split_pair(spec, llr, L, what)
    for L in TIE_LISTS:
        spec, q, want = tie_case(L)
        full_and_unequal(want, L, 64, f"ties L={L}")
        assert any(len(set(want[3][b, :L].tolist())) < L for b in range(len(q))), "no equal metrics"
        if L % 2:
            plain_split_pair(spec, q, L, f"ties L={L}")
    spec, llr, want = reuse_case()
    full_and_unequal(want, REUSE_L, 32, "state reuse")
    plain_split_pair(spec, llr, REUSE_L, "state reuse")
    for n, L in Q8_LDS:
        spec, rows, want, share, pairs = q8_lds_case(n, L)
        full_and_unequal(want, L, 1 << (n - 1), f"q8 n={n} L={L}")
        assert share > 0 and (pairs > 0 or L % 2 == 0), (n, L, share, pairs)
    for n, K, dyn, punct, L in Q8_TIERED:
        spec, rows, few, share, pairs = q8_tiered_case(n, K, dyn, punct, L)
        full_and_unequal(few, L, K, f"tiered q8 n={n} L={L}")
        assert share > 0 and (pairs > 0 or L % 2 == 0), (n, L, share, pairs)
    for layers, K, dyn, punct, L in MIXED:
        if not is_named(layers):
            spec, B, snr, seed = mixed_case(layers, K, dyn, punct, L)
            o = PolarOracle(spec, kernel_dir())
            full_and_unequal(o.decode_batch(words(o, K, B, snr, seed), L), L, K, f"{'-'.join(layers)} L={L}")
    for layers, K, dyn, punct, L in BUDGET:
        for snr in (0.0, 2.0):
            spec, o, llr = budget_case(layers, K, dyn, punct, L, snr)
            full_and_unequal(o.decode_batch(llr, L), L, K, f"budget L={L} {snr} dB")


# ================================================================ 2. the recorded lists

LIST_FIXTURES = ["lists_arikan_n6", "lists_arikan_n7_ties", "lists_bch8_A", "lists_dyn_arikan_n7_a33"]


def list_fixture(name):
    return R.load_fixture(os.path.join(R.GOLD, f"polar_ref_{name}.txt.gz"))


def test_list_fixtures_are_what_they_are_for():
    """The four codes of the issue, every L of LISTS, data no larger than the largest other
    polar_ref_* fixture; ties and zeros in the tie fixture, more than 32 constraints live in the
    dense one, and every list size recorded with a full list somewhere."""
    import dense_codes
    from polar_lib import max_active
    files = R.fixture_files("code") + R.fixture_files("trellis") + R.fixture_files("counts") + R.fixture_files("capacity")
    ours = [p for p in files if os.path.basename(p).startswith("polar_ref_lists_")]
    assert sorted(os.path.basename(p)[len("polar_ref_"):-len(".txt.gz")] for p in ours) == LIST_FIXTURES
    assert max(os.path.getsize(p) for p in ours) <= max(os.path.getsize(p) for p in files if p not in ours)
    assert list_fixture("lists_arikan_n6").spec == arikan_spec(6, 32, dyn=5, punct=(1, 7), seed=6)
    t = list_fixture("lists_arikan_n7_ties")
    assert t.spec == arikan_spec(7, 64, dyn=4, seed=77) and np.all(t.llr % 4 == 0) and np.any(t.llr == 0)
    assert list_fixture("lists_bch8_A").spec.split("\n")[1] == "-bch8.txt A"
    d = list_fixture("lists_dyn_arikan_n7_a33")
    assert d.spec == dense_codes.spec("dyn_arikan_n7_a33") and max_active(d.spec) == 33
    for name in LIST_FIXTURES:
        fx = list_fixture(name)
        assert fx.list_sizes == list(LISTS)
        for L in LISTS:
            rows = fx.decoded(L)
            assert any(c == L for c, *_ in rows) and any(len(set(m.tolist())) > 1 for *_, m in rows), (name, L)
        assert any(len(set(m.tolist())) < len(m) for *_, m in t.decoded(7))


@pytest.mark.gpu
@pytest.mark.parametrize("L", LISTS)
def test_gpu_8x8_layer_through_the_trellis_matches_reference(L, tmp_path, monkeypatch):
    """The reference takes every matrix kernel through its trellis processor; the GPU enumerates an
    8 x 8 one unless told otherwise (BCHK_POLAR_TRELLIS)."""
    from test_polar_reference import assert_lists_equal
    monkeypatch.setenv("BCHK_POLAR_TRELLIS", "2")
    fx = list_fixture("lists_bch8_A")
    fx.write_kernels(str(tmp_path))
    d = load().PolarListDecoder(fx.spec, L, kernel_dir=str(tmp_path))
    got = d.decode(fx.llr)
    d.close()
    assert_lists_equal(got, fx.decoded(L), f"GPU trellis lists_bch8_A L={L}")


# ================================================================ 3. the f32 all-Arikan kernels

def _id5(c):
    return f"A{c[0]}-K{c[1]}-L{c[4]}"


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,dyn,punct,L", F32_LDS, ids=[_id5(c) for c in F32_LDS])
def test_gpu_sclist_matches_oracle(n, K, dyn, punct, L):
    spec, llr, want = f32_case(n, K, dyn, punct, L)
    assert_same(gpu_decoder(spec, L).decode(llr), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,dyn,punct,L", F32_TIERED, ids=[_id5(c) for c in F32_TIERED])
def test_gpu_tiered_every_split(n, K, dyn, punct, L):
    """Every boundary 1..n against the oracle, and so against the LDS kernel on the same rows."""
    spec, llr, want = f32_case(n, K, dyn, punct, L)
    for split in range(1, n + 1):
        d = tiered(spec, L, split)
        assert d.split == split
        got = d.decode(llr)
        d.close()
        assert_same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("L", TIE_LISTS)
def test_gpu_ties_and_zeros(L):
    """Equal metrics and zero LLRs: the (score, index) order decides, and only path indices may
    break ties, never array indices."""
    spec, q, want = tie_case(L)
    assert_same(gpu_decoder(spec, L).decode(q), want)
    for split in (1, 3, 7):
        d = tiered(spec, L, split)
        got = d.decode(q)
        d.close()
        assert_same(got, want)


@pytest.mark.gpu
def test_gpu_tiered_state_reuse_across_codewords(monkeypatch):
    """Three waves decode 1000 codewords each at L = 7: nothing of a codeword's arrays, indices or
    free-array masks may reach the next."""
    monkeypatch.setenv("BCHK_POLAR_GRID", "3")
    spec, llr, want = reuse_case()
    d = tiered(spec, REUSE_L, 6)
    assert d.state_info()["grid"] == 3
    got = d.decode(llr)
    d.close()
    assert_same(got, want)


def f32_restated_layout(n, L, K, split):
    """(lds_bytes, workspace_bytes) of polar_tiered_layout, from DESIGN 5.15: per path S of the
    sub-code as floats (a multiple of 4, plus 4), the packed C words past the split on an odd
    stride; idx and own as bytes; act and rec; the workspace's float layers and packed words."""
    U = 1 << n
    cwsplit = q8_restated_layout(n, L, K, split)[2]
    cwall = sum(((U if lam == 0 else U >> (lam - 1)) + 31) // 32 for lam in range(n + 1))
    Us = U >> split
    pathS = ((Us + 3) & ~3) + 4 if Us > 1 else 0
    nC = cwall - cwsplit
    pathC = nC | 1 if nC else 0
    o_own = 4 * pathS * L + 4 * pathC * L + split * L
    o_act = (o_own + L + 15) & ~15
    lds = (o_act + 4 * L + 4 * L * max((K + 31) // 32, 1) + 15) & ~15
    w_C = (4 * L * (U - Us) + 15) & ~15
    return lds, (w_C + 4 * L * cwsplit + 255) & ~255


def f32_restated_split(n, L, K):
    def lds(s):
        return f32_restated_layout(n, L, K, s)[0]

    def waves(s):
        return min(8, LDS_MAX // lds(s))

    s = 1
    while s < n and lds(s) > LDS_MAX:
        s += 1
    while s < n and waves(s + 1) > waves(s):
        s += 1
    return s


def test_restated_f32_layout_gives_the_pinned_sizes():
    """The restatement itself, on the CPU: test_polar_tiered.AUTO_CHOICE holds what an MI355X
    reported at powers of two."""
    for (n, L, ask), want in AUTO_CHOICE.items():
        K = 1 << (n - 1)
        split = f32_restated_split(n, L, K) if ask is None else ask
        assert (split,) + f32_restated_layout(n, L, K, split) == want, (n, L, ask)


LAYOUT_SHAPES = [(10, None), (10, 4), (11, None), (12, None), (12, 3), (13, None), (13, 5), (14, None), (14, 6)]  # n, split asked


@pytest.mark.gpu
@pytest.mark.parametrize("L", LAYOUT_LISTS)
def test_gpu_tiered_layouts_and_auto_split(L):
    """state_info() against both restated layouts, byte tables idx[split L] and own[L] that end off
    a word boundary included: creation only, nothing is decoded."""
    for n, ask in LAYOUT_SHAPES:
        K = 1 << (n - 1)
        spec = arikan_spec(n, K)
        for make, layout, rule in ((tiered, f32_restated_layout, f32_restated_split),
                                   (tiered_q8, lambda *a: q8_restated_layout(*a)[:2], q8_restated_split)):
            d = make(spec, L, ask)
            st = d.state_info()
            d.close()
            split = rule(n, L, K) if ask is None else ask
            lds, ws = layout(n, L, K, split)
            assert (st["split"], st["lds_bytes"], st["workspace_bytes"]) == (split, lds, ws), (make.__name__, n, L, ask)
            assert lds <= LDS_MAX


@pytest.mark.gpu
def test_gpu_tiered_past_the_lds_limit_at_list_24():
    """(2048, 1024) at L = 24: 24 paths of 2048 floats are 192 KiB, past the 160 KiB of LDS."""
    n, K, L = PAST_LDS
    F = load()
    with pytest.raises(F.BchkError, match="LDS"):
        F.PolarListDecoder(arikan_spec(n, K, dyn=8, seed=n), L)
    spec, o, info, llr = workload(n, K, 8, (), 1.5, 8, seed=n + L)
    want = o.decode_batch(llr, L)
    assert (want[0] == L).all()
    d = tiered(spec, L)
    got = d.decode(llr)
    d.close()
    assert_same(got, want)


# ================================================================ 4. the int8 kernels

@pytest.mark.gpu
@pytest.mark.parametrize("n,L", Q8_LDS)
def test_gpu_q8_matches_restatement_with_saturation(n, L):
    spec, rows, want, share, _ = q8_lds_case(n, L)
    print(f"U={1 << n} L={L}: {100 * share:.1f} % of the g steps clamp")
    assert share > 0
    assert q8_check(spec, rows, L) == share  # the GPU's lists against the restatement's, computed afresh
    q8_assert_same(q8_decoder(spec, L).decode(rows), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,dyn,punct,L", Q8_TIERED, ids=[_id5(c) for c in Q8_TIERED])
def test_gpu_q8_tiered_every_split(n, K, dyn, punct, L):
    """Every boundary 1..n against the LDS int8 decoder, whose first rows are the restatement's."""
    spec, rows, few, share, _ = q8_tiered_case(n, K, dyn, punct, L)
    assert share > 0
    with q8_context(spec, L) as d:
        want = d.decode(rows)
    q8_assert_same(tuple(a[:Q8_TIERED_RESTATED] for a in want), few)
    for split in range(1, n + 1):
        d = tiered_q8(spec, L, split)
        assert d.split == split
        got = d.decode(rows)
        d.close()
        q8_assert_same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,L", Q8_NARROW)
def test_gpu_q8_layers_narrower_than_a_word(n, K, L):
    spec = arikan_spec(n, K)
    rows = np.random.default_rng(n).integers(-128, 128, (40, 1 << n)).astype(np.int8)
    rows[0] = 0
    want = restated(spec, rows, L)
    assert (want[0] == min(L, 1 << K)).all()
    for label, state, split in q8_states(spec):
        with q8_context(spec, L, state, split) as d:
            q8_assert_same(d.decode(rows), want)


@pytest.mark.gpu
def test_gpu_q8_sweep_equals_its_own_pipeline():
    from test_polar_q8 import SWEEP_B, SWEEP_QMAX, SWEEP_SCALE, SWEEP_SEED
    with q8_context(arikan_spec(6, 32, dyn=5, punct=(1, 7), seed=3), Q8_SWEEP_L) as d:
        want, flags = pipeline(d, "awgn", 1.0, SWEEP_B, SWEEP_SEED)
        recs, secs, nwords = d.sweep_device(1.0, 0.5, 1, SWEEP_B, SWEEP_B + 1, seed=SWEEP_SEED, batch=SWEEP_B,
                                            channel="awgn", scale=SWEEP_SCALE, qmax=SWEEP_QMAX)
    assert recs == [(1.0, want)] and nwords == SWEEP_B and secs > 0
    assert want[0] == SWEEP_B and want[1] == int((flags & 1).sum()) > 3


# ================================================================ 5. the mixed-kernel decoders

@pytest.mark.gpu
@pytest.mark.parametrize("layers,K,dyn,punct,L", MIXED, ids=["-".join(c[0]) + f"-L{c[4]}" for c in MIXED])
def test_gpu_mixed_and_tiered_mixed_every_split(layers, K, dyn, punct, L):
    """polar_mixed (LDS) and polar_mixed_tiered at every split against the C oracle; with a named
    layer, as tests/test_polar_named_kernels.py stands at L > 1, the LDS kernel is the tiered
    one's reference and nothing is claimed about the compiled library."""
    spec, B, snr, seed = mixed_case(layers, K, dyn, punct, L)
    check_every_split(spec, kernel_dir(), L, B, snr, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("layers,K,dyn,punct,L", BUDGET, ids=[f"L{c[4]}" for c in BUDGET])
def test_gpu_tiny_budget_forced_search_matches_oracle(layers, K, dyn, punct, L, monkeypatch):
    """Every search round (then: every item) a suspension: the save slot carries L lanes' registers
    and the LDS of L paths."""
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 17 + K)
    one = _decoder(monkeypatch, spec, L, kernel_dir(), "0", ml=2)
    tiny = _decoder(monkeypatch, spec, L, kernel_dir(), TINY, ml=2)
    try:
        for snr in (0.0, 2.0):
            _, o, llr = budget_case(layers, K, dyn, punct, L, snr)
            want = o.decode_batch(llr, L)
            a = _decode(monkeypatch, one, llr)
            assert one.last_launches() == 1
            assert_same(a, want)
            for no_mid in (False, True):
                b = _decode(monkeypatch, tiny, llr, no_mid)
                assert tiny.last_launches() > 1
                assert_same(b, want)
    finally:
        one.close()
        tiny.close()


# ================================================================ 6. the output contract

def short_specs(K):
    """An all-Arikan code (lds, tiered, tiered_mixed, q8, tiered_q8) and one with a matrix layer
    (the mixed LDS kernel, tiered_mixed) of 16 symbols and 2^K codewords."""
    return arikan_spec(4, K), mixed_spec(("k4", "A", "A"), K, seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("K,L,count", SHORT, ids=[f"K{c[0]}-L{c[1]}" for c in SHORT])
def test_gpu_short_lists_leave_the_other_rows_and_the_guards(K, L, count, monkeypatch):
    """2^K < L: count = 2^K, the first rows the reference's, every other row of info, cw and metric
    still the sentinel, the guards intact; both entry points, every state at every split; 70 words
    over 3 workgroups, which reuse their state from word to word."""
    monkeypatch.setenv("BCHK_POLAR_GRID", "3")
    for spec in short_specs(K):
        llr = batches(spec, 70, seed=11)[0]
        want = oracle(spec).decode_batch(llr, L)
        assert (want[0] == count).all()
        for label, state, split in states(spec):
            with context(spec, L, state, split) as d:
                assert d.state_info()["grid"] == 3
                for fn in (decode_device, decode_host):
                    assert_strict(fn(d, llr), want, f"K={K} L={L} {label} {fn.__name__}")
    spec = short_specs(K)[0]
    rows = uniform_rows(70, 16, seed=11 + K)
    want = restated(spec, rows, L)
    assert (want[0] == count).all()
    for label, state, split in q8_states(spec):
        with q8_context(spec, L, state, split) as d:
            assert d.state_info()["grid"] == 3
            for how, fn in Q8_ENTRIES:
                assert_strict(fn(d, rows), want, f"K={K} L={L} {label} {how}")


NULL_CW = [("A7-N128", "lds", None), ("A7-N128", "tiered", 3), ("A7-N128", "tiered_mixed", 4),
           ("bch16_A-N32", "lds", None), ("bch16_A-N32", "tiered_mixed", 2)]


@pytest.mark.gpu
def test_gpu_cw_null():
    """d_cw = 0 / cw = NULL at L = 5: count, info and metric the reference's, and a sentinel-filled
    buffer that is not passed stays as it is."""
    L = NULL_L
    for name, state, split in NULL_CW:
        spec = NULL_CW_SPECS[name]()
        llr = batches(spec, seed=13)[1]
        want = oracle(spec).decode_batch(llr, L)
        with context(spec, L, state, split) as d:
            for fn in (decode_device, decode_host):
                assert_strict(fn(d, llr), want, f"{name} {state} {fn.__name__}")
                assert_strict(fn(d, llr, cw=False), want, f"{name} {state} {fn.__name__} cw = NULL", cw=False)
    spec = NULL_CW_SPECS["A7-N128"]()
    rows = noisy_rows(spec, 12, 2.0, seed=13)
    want = restated(spec, rows, L)
    for state, split in (("lds", None), ("tiered_q8", 3)):
        with q8_context(spec, L, state, split) as d:
            for how, fn in Q8_ENTRIES:
                assert_strict(fn(d, rows), want, f"q8 {state} {how}")
                assert_strict(fn(d, rows, cw=False), want, f"q8 {state} {how} cw = NULL", cw=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE_K))
def test_gpu_dimension_zero_and_nothing_frozen(name):
    """K = 0: one row, the frozen word; K = U: L = 3 of the 2^16 words. Every state, both entry
    points."""
    L = EDGE_L
    spec = EDGE_K[name][0]()
    K = header(spec)[1]
    count = min(L, 1 << K)
    llrs = batches(spec, 12, seed=5)
    wants = [oracle(spec).decode_batch(llr, L) for llr in llrs]
    for label, state, split in states(spec):
        with context(spec, L, state, split) as d:
            for fn in (decode_host, decode_device):
                for i, (llr, want) in enumerate(zip(llrs, wants)):
                    assert (want[0] == count).all()
                    assert_strict(fn(d, llr), want, f"{name} {label} {fn.__name__} batch {i}")
    rows = uniform_rows(12, 16, seed=K + 2)
    want = restated(spec, rows, L)
    assert (want[0] == count).all()
    for label, state, split in q8_states(spec):
        with q8_context(spec, L, state, split) as d:
            for how, fn in Q8_ENTRIES:
                assert_strict(fn(d, rows), want, f"{name} {label} {how}")


def sim_decoder(L):
    from test_polar_sim import SIM_CODE
    n, K, dyn, punct = SIM_CODE
    return load().PolarListDecoder(arikan_spec(n, K, dyn=dyn, punct=punct, seed=3), L)


@pytest.mark.gpu
def test_gpu_count_device_walks_seven_rows():
    """bchk_polar_count_device at L = 7 against include/bchk.h's table in numpy, words without a
    decision among them; the list-error counter walks rows 1 .. count - 1 of stride-7 lists."""
    import torch
    from test_polar_sim import SNR, Batch, _sync, _zeros, np_counters
    d = sim_decoder(COUNT_L)
    B = 256
    bt = Batch(d, SNR, B, 1)
    out8, flags = _zeros((8,), torch.int64), _zeros((B,), torch.uint8)
    _sync()
    bt.count_device(0, B, out8, flags)
    per, want_flags = np_counters(*bt.host())
    np.testing.assert_array_equal(out8.cpu().numpy(), per.sum(axis=0))
    np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)
    blk, lst = int(per[:, 1].sum()), int(per[:, 5].sum())
    assert 0 < lst < blk, (blk, lst)  # some sent words lie further down the list, some in no row
    bt.count[::3] = 0
    bt.count[1::7] = -1
    out8, flags = _zeros((8,), torch.int64), _zeros((B,), torch.uint8)
    _sync()
    bt.count_device(0, B, out8, flags)
    per, want_flags = np_counters(*bt.host())
    assert per[:, 7].sum() > 80
    np.testing.assert_array_equal(out8.cpu().numpy(), per.sum(axis=0))
    np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)
    d.close()


@pytest.mark.gpu
def test_gpu_sweep_matches_word_by_word_loop():
    """bchk_polar_sweep_device (f32, AWGN) at L = 6: two points cut by errors, three batch sizes."""
    from test_polar_sim import SNR, _reference_sweep
    d = sim_decoder(SWEEP_L)
    runs = {b: d.sweep_device(SNR, 0.5, 2, 1500, 20, seed=5, batch=b) for b in (64, 37, 1500)}
    want, _ = _reference_sweep(d, SNR, 0.5, 2, 1500, 20, 5)
    for b, (recs, secs, nwords) in runs.items():
        assert recs == want, b
        assert secs > 0 and nwords >= sum(c[0] for _, c in recs)
    assert any(c[1] == 20 and c[0] < 1500 for _, c in want)
    d.close()
