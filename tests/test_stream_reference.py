"""The counter-based channel streams against an independent reference (tests/philox_lib.py):
the BCH front-end (chan_kernel), the polar front-end (polar_gen_kernel) and the sampled BEC
design (draw_rank) all draw from csrc/bchk_philox.h, and the other suites check that generator
only statistically and against itself. Here the documented counter layouts are restated in
numpy / Python integers and the device output is compared element for element: information
bits, codewords and BEC patterns bit for bit, the Gaussian noise against a Box-Muller evaluated
well above double precision. bchk_sweep_device's cut at the e-th frame error is replayed word by
word on the host.

Tolerance on the noise (a relative error on z against the high-precision reference). The
derivation assumes the double-precision bounds of the ROCm device library as its public HIP
math documentation states them -- log <= 1 ulp, sqrt <= 1 ulp, sincospi <= 2 ulp: rad = sqrt(-2
log u1) is within 1.5 * 2^-52 relative (the square root halves the logarithm's error), the
sine / cosine adds 2 * 2^-52, the product 0.5 * 2^-52: about 4 * 2^-52 on z. The asserted bound
is 2^-49, twice that; the slack covers the binade dependence of ulp-to-relative conversion and a
last-bit difference between the host's and numpy's sd / sigma. The three library bounds could
NOT be confirmed from an installed ROCm tree: its HIP headers (amd_detail/math_fwd.h) only
declare the __ocml_* entry points and carry no accuracy table, and no copy of the HIP math
documentation is installed with it, so the figures above are the documented ones as recalled and
the sum was not redone. The BCH tests print the largest observed error in units of 2^-52 |z|
(taken where sd |z| >= |y|, so that the final rounding of y adds at most 0.5): 1.62 on the
MI355X over the six batches below, against the derived 4 and the asserted 8.
"""
import functools
import math
import os
from decimal import Decimal

import numpy as np
import pytest

import philox_lib as P
from bchk_pkg import load
from oracle_lib import Oracle
from polar_lib import PolarOracle, arikan_spec

SEED = 5
BCH_CODES = [(4, 2, 1.0), (6, 6, 3.0), (7, 10, 5.0), (8, 15, 6.0)]  # m, t, Eb/N0
BCH_B, BCH_WORD0 = 300, 123
# (6, 6) only: the word index / the pair index G / 2 crosses 2^32 inside the batch
BCH_EDGES = [(1 << 32) - 70, (1 << 33) // 63 - 100]
BCH_EDGE_B = 200

POLAR_SNR, POLAR_B = 1.0, 130
POLAR_SPECS = {
    "n9k300": lambda: arikan_spec(9, 300, dyn=5, seed=9),            # U = N = 512: blocks 128 + 128 + 44
    "n6punct": lambda: arikan_spec(6, 32, dyn=5, punct=(1,), seed=3),  # N = 63: pairs straddle words
}
POLAR_CASES = [("n9k300", 77), ("n6punct", 77), ("n6punct", (1 << 32) - 3),
               ("n6punct", (1 << 33) // 63 - 60)]  # the last: the pair index crosses 2^32

BEC_CASES = [("ebch16", 8), ("ebch64", 20), ("ebch64", 32)]
BEC_SAMPLES, BEC_SEED = 4096, 3


# ---------------------------------------------------------------- shared references

@functools.lru_cache(maxsize=None)
def bch_ref(m, t, snr, word0, B):
    o = Oracle(m, t)
    return o, P.bch_words(o.g, o.n, o.k, snr, SEED, word0, B)


@functools.lru_cache(maxsize=None)
def polar_ref(name, word0):
    spec = POLAR_SPECS[name]()
    o = PolarOracle(spec)
    info, cw, llr = P.polar_words(o.encode, o.N, o.K, POLAR_SNR, SEED, word0, POLAR_B)
    return spec, info, cw, llr, P.llr_float32(llr)


@functools.lru_cache(maxsize=None)
def bec_ref(l, w):
    return P.bec_draw(l, w, BEC_SEED, np.arange(BEC_SAMPLES, dtype=np.uint64))


# ---------------------------------------------------------------- CPU: the reference itself

def test_philox_known_answer_vectors():
    """The Random123 known-answer vectors of philox4x32-10."""
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for ctr, key, want in kat:
        assert tuple(int(v[0]) for v in P.philox4x32_10(ctr, key)) == want
    # vectorised: the three at once
    got = P.philox4x32_10([np.array([k[0][i] for k in kat]) for i in range(4)],
                          [np.array([k[1][i] for k in kat]) for i in range(2)])
    assert [tuple(int(g[j]) for g in got) for j in range(3)] == [k[2] for k in kat]


def test_unit53_range_and_bits():
    assert int(P.unit53_int(0, 0)) == 1 and float(P.unit53(0, 0)) == 2.0 ** -53
    assert int(P.unit53_int(0xFFFFFFFF, 0xFFFFFFFF)) == 1 << 53 and float(P.unit53(0xFFFFFFFF, 0xFFFFFFFF)) == 1.0
    assert int(P.unit53_int(1, 0)) == (1 << 21) + 1      # a is the high word
    assert int(P.unit53_int(0, 1 << 11)) == 2            # the top 21 bits of b, the low 11 dropped
    assert int(P.unit53_int(0, (1 << 11) - 1)) == 1


FORCED = [(1, 12345), (1 << 53, 999), (1 << 53, 1 << 53)] + \
         [(v1, q << 51) for v1 in (1, 3 << 50, (1 << 53) - 1) for q in (1, 2, 3, 4)]


@pytest.mark.skipif(not P.HAVE_LD, reason="np.longdouble is a double here: the decimal path is the reference")
def test_longdouble_pair_matches_50_digit_decimal():
    """256 counters and the forced inputs: u1 = 2^-53, u1 = 1 (z = 0 exactly), u2 in {1/4, 1/2,
    3/4, 1}, whose zeros and +-1 come out exact."""
    v1, v2 = P.pair_units(np.arange(256, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15), SEED)
    v1 = np.concatenate([v1, np.array([f[0] for f in FORCED], np.uint64)])
    v2 = np.concatenate([v2, np.array([f[1] for f in FORCED], np.uint64)])
    z0, z1 = P.normal_from_units_ld(v1, v2)
    worst = Decimal(0)
    for i in range(len(v1)):
        d0, d1 = P.normal_from_units_dec(v1[i], v2[i])
        for got, want in ((z0[i], d0), (z1[i], d1)):
            got = P.ld_to_decimal(got)
            if want == 0:
                assert got == 0
                continue
            rel = abs(got - want) / abs(want)
            worst = max(worst, rel)
            assert rel <= Decimal(2) ** -60, (i, int(v1[i]), int(v2[i]), got, want)
    print("longdouble against decimal: worst relative error 2^%.1f" % math.log2(float(worst)))
    # the exact special values
    for v1f, v2f in FORCED:
        a, b = (float(v[0]) for v in P.normal_from_units_ld(v1f, v2f))
        d0, d1 = P.normal_from_units_dec(v1f, v2f)
        if v1f == 1 << 53:
            assert a == 0 and b == 0 and d0 == 0 and d1 == 0
        q = v2f >> 51
        if q << 51 == v2f:
            z0, z1 = P.normal_from_units_ld(v1f, v2f)
            rad, rad_dec = P.normal_from_units_ld(v1f, 1 << 53)[0][0], P.normal_from_units_dec(v1f, 1 << 53)[0]
            assert abs(float(rad) - math.sqrt(-2 * math.log(v1f * 2.0 ** -53))) <= 2.0 ** -51 * float(rad)
            want = {1: (0, 1), 2: (-1, 0), 3: (0, -1), 4: (1, 0)}[q]
            for got, dec, w in ((z0[0], d0, want[0]), (z1[0], d1, want[1])):
                if w == 0:
                    assert got == 0 and dec == 0
                else:  # +-rad: exactly the radius, no trigonometric error
                    assert got == w * rad
                    assert dec.copy_abs() == rad_dec and dec.is_signed() == (w < 0)
    # u1 = 2^-53: the largest radius the generator can give
    assert abs(float(P.normal_from_units_ld(1, 1 << 53)[0][0]) - math.sqrt(2 * 53 * math.log(2))) < 1e-14


def test_decimal_path_stands_in_for_longdouble():
    """Where np.longdouble is a double the streams take their noise from the decimal path on
    DEC_WORDS words: the two paths give the same words here."""
    o = Oracle(4, 2)
    tx, y, z = P.bch_words(o.g, o.n, o.k, 1.0, SEED, 123, 8, use_ld=False)
    assert y.shape == (P.DEC_WORDS, o.n) and y.dtype == object
    if P.HAVE_LD:
        tx2, y2, z2 = P.bch_words(o.g, o.n, o.k, 1.0, SEED, 123, 8)
        np.testing.assert_array_equal(tx, tx2)
        for a, b in zip(z.ravel(), z2[:P.DEC_WORDS].ravel()):
            assert abs(P.ld_to_decimal(b) - a) <= Decimal(2) ** -60 * abs(a)
        for a, b in zip(y.ravel(), y2[:P.DEC_WORDS].ravel()):  # y = +-1 + sd z may cancel
            assert abs(P.ld_to_decimal(b) - a) <= Decimal(2) ** -60 * (1 + abs(a))
    f32, dec = P.llr_float32(y)
    assert dec.all() and f32.dtype == np.float32


def test_bec_draw_ranks_weights_and_rejections():
    for name, w in BEC_CASES:
        l = 16 if name == "ebch16" else 64
        pats, ranks, attempts, cands = bec_ref(l, w)
        total = math.comb(l, w)
        assert all(0 <= r < total for r in ranks)
        assert all(bin(int(p)).count("1") == w and int(p) < 1 << l for p in pats)
        assert len(set(ranks)) > 0.8 * len(ranks)
        if (l, w) == (16, 8):  # both retry paths are in the GPU comparison
            assert any(c == 1 for c in cands) and any(a >= 1 for a in attempts)
            assert any(a >= 1 and c == 1 for a, c in zip(attempts, cands))
            print("bec_draw(16, 8): second candidate %d, later attempt %d of %d"
                  % (sum(cands), sum(a >= 1 for a in attempts), len(ranks)))
    # colex order: rank 0 is the w lowest elements, the last rank the w highest
    assert P.unrank_colex(16, 8, 0) == 0xFF and P.unrank_colex(16, 8, math.comb(16, 8) - 1) == 0xFF00
    assert [P.unrank_colex(4, 2, r) for r in range(6)] == [0b0011, 0b0101, 0b0110, 0b1001, 0b1010, 0b1100]


def test_bch_reference_words_are_codewords():
    from test_channel import _gf2_mod
    for m, t, snr in BCH_CODES:
        o, (tx, y, z) = bch_ref(m, t, snr, BCH_WORD0, BCH_B)
        assert tx.shape == (BCH_B, o.n) and not _gf2_mod(tx, o.g).any()
        assert 0.4 < tx.mean() < 0.6


def test_polar_batches_have_no_undecidable_llr():
    """Decidability depends on the reference alone: the chosen seed leaves no element of any
    batch whose float32 the 2^-48 interval does not settle."""
    for name, word0 in POLAR_CASES:
        spec, info, cw, llr, (f32, decidable) = polar_ref(name, word0)
        assert int((~decidable).sum()) == 0, (name, word0)
        assert 0.4 < info.mean() < 0.6


# ---------------------------------------------------------------- GPU: the BCH stream

def _gpu_bch(d, snr, B, word0):
    import torch
    dtx = torch.zeros((B, d.n), dtype=torch.uint8, device="cuda")
    dy = torch.zeros((B, d.n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d.generate_device(snr, B, dtx.data_ptr(), dy.data_ptr(), seed=SEED, word0=word0)
    d.sync()
    return dtx.cpu().numpy(), dy.cpu().numpy()


def _check_bch(m, t, snr, word0, B):
    d = load().KanekoKernelProcessor(m, t, J=15)
    o, (tx_ref, y_ref, z_ref) = bch_ref(m, t, snr, word0, B)
    assert (d.n, d.k) == (o.n, o.k) and np.array_equal(d.g, o.g)
    tx, y = _gpu_bch(d, snr, B, word0)
    np.testing.assert_array_equal(tx, tx_ref)
    R = len(y_ref)
    sd = P.lift(np.float64(P.bch_sd(o.n, o.k, snr)))
    noise = abs(sd * z_ref)
    err = abs(P.lift(y[:R]) - y_ref)
    # units of 2^-52 |z| where the noise dominates y (the final rounding of y adds <= 0.5 there)
    big = noise >= abs(y_ref)
    units = max(float(v) for v in (err[big] / (P.lift(np.float64(2.0 ** -52)) * noise[big])))
    print("BCH(%d,%d) word0 %d: max |z_gpu - z_ref| / (2^-52 |z_ref|) = %.3f over %d elements"
          % (o.n, o.k, word0, units, int(big.sum())))
    bound = P.lift(np.float64(2.0 ** -49)) * noise + P.lift(np.float64(2.0 ** -52)) * np.maximum(abs(y_ref), noise)
    bad = np.argwhere(~(err <= bound))
    assert not len(bad), (bad[:5].tolist(), [float(err[tuple(i)]) for i in bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("m,t,snr", BCH_CODES)
def test_gpu_bch_stream_matches_reference(m, t, snr):
    """B = 300 from an odd word: one full workgroup (4 waves of 64 words), a second one whose
    last wave has 44 rows, odd element bases where Box-Muller pairs straddle the wave blocks."""
    _check_bch(m, t, snr, BCH_WORD0, BCH_B)


@pytest.mark.gpu
@pytest.mark.parametrize("word0", BCH_EDGES, ids=["word-crosses-2^32", "pair-crosses-2^32"])
def test_gpu_bch_stream_high_counter_words(word0):
    n = 63
    assert word0 < 1 << 32 < word0 + BCH_EDGE_B or (word0 * n) >> 1 < 1 << 32 < ((word0 + BCH_EDGE_B) * n) >> 1
    _check_bch(6, 6, 3.0, word0, BCH_EDGE_B)


# ---------------------------------------------------------------- GPU: the polar stream

@pytest.mark.gpu
@pytest.mark.parametrize("name,word0", POLAR_CASES)
def test_gpu_polar_stream_matches_reference(name, word0):
    from test_polar_sim import generate
    spec, info_ref, cw_ref, llr_ref, (f32, decidable) = polar_ref(name, word0)
    d = load().PolarListDecoder(spec, 1)
    assert (d.N, d.K) == cw_ref.shape[1:] + info_ref.shape[1:]
    info, cw, llr = generate(d, POLAR_SNR, POLAR_B, seed=SEED, word0=word0)
    np.testing.assert_array_equal(info, info_ref)
    np.testing.assert_array_equal(cw, cw_ref)  # = PolarOracle.encode(info)
    R = len(f32)
    skipped = int((~decidable).sum())
    assert skipped <= 1
    got, want = llr[:R].view(np.uint32), f32.view(np.uint32)
    bad = np.argwhere((got != want) & decidable)
    assert not len(bad), (bad[:5].tolist(), [(float(llr[tuple(i)]), float(f32[tuple(i)])) for i in bad[:5]])


# ---------------------------------------------------------------- GPU: the BEC draws

def _bec_kernel(name):
    return load().kernel_ebch(4 if name == "ebch16" else 6)


@pytest.mark.gpu
@pytest.mark.parametrize("name,w", BEC_CASES)
def test_gpu_bec_draws_match_reference(name, w):
    K = _bec_kernel(name)
    want = bec_ref(len(K), w)[0]
    unc, tried, exact, pat = load().kernel_bec_sample(K, BEC_SAMPLES, seed=BEC_SEED, pattern_weight=w)
    assert not exact[w] and int(tried[w]) == BEC_SAMPLES
    np.testing.assert_array_equal(pat, want)


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["1", "37"])
def test_gpu_bec_draws_do_not_depend_on_the_lane_shape(run):
    """BCHK_BEC_RUN = patterns per lane: a lane's first and its later patterns both come from
    the sample index."""
    K = _bec_kernel("ebch16")
    want = bec_ref(16, 8)[0]
    old = os.environ.get("BCHK_BEC_RUN")
    os.environ["BCHK_BEC_RUN"] = run
    try:
        pat = load().kernel_bec_sample(K, BEC_SAMPLES, seed=BEC_SEED, pattern_weight=8)[3]
    finally:
        if old is None:
            del os.environ["BCHK_BEC_RUN"]
        else:
            os.environ["BCHK_BEC_RUN"] = old
    np.testing.assert_array_equal(pat, want)


# ---------------------------------------------------------------- GPU: bchk_sweep_device replayed

SWEEP_P, SWEEP_E, SWEEP_MAX_SNR, SWEEP_SEED = 3000, 40, 1.0, 7
SWEEP_BATCHES = (64, 37, 3000)
CHUNK = 500


def _replay_sweep(d, decode, p, e, max_snr, seed):
    """fun()'s loop (src/dataForPlot.cpp:41-95) word by word over the device stream: a point
    ends with the word carrying the e-th frame error or after p words, the next starts at the
    following word; the bit-error count is never reset; a word that is never accepted is
    compared against the previous decision. -> (CSV lines as lists of %g fields, how each point
    was cut, never-accepted words)."""
    n = d.n
    lines, cuts = [], []
    word = count_e = never = 0
    decoded = np.zeros(n, np.uint8)
    stnr = 0.0
    while stnr <= max_snr:
        count = count_err = 0
        D = Cc = Ss = 0
        while count < p and count_err < e:
            nb = min(CHUNK, p - count)
            tx, y = _gpu_bch_seed(d, stnr, nb, word, seed)
            res, acc, ops = decode(y)
            used = 0
            for b in range(nb):
                if acc[b]:
                    decoded = res[b]
                else:
                    never += 1
                diff = tx[b] != decoded
                count_err += int(diff.any())
                count_e += int(diff.sum())
                D, Cc, Ss = D + int(ops[b][0]), Cc + int(ops[b][1]), Ss + int(ops[b][2])
                count += 1
                used += 1
                if count_err >= e:
                    break
            word += used
        vals = (stnr, count_err / count, count_e / count / n, D / count, Cc / count, Ss / count)
        lines.append(["%g" % v for v in vals])  # ostream defaults: %g, 6 significant digits
        cuts.append("errors" if count_err >= e else "words")
        stnr += 0.5
    return lines, cuts, never


def _gpu_bch_seed(d, snr, B, word0, seed):
    import torch
    dtx = torch.zeros((B, d.n), dtype=torch.uint8, device="cuda")
    dy = torch.zeros((B, d.n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d.generate_device(snr, B, dtx.data_ptr(), dy.data_ptr(), seed=seed, word0=word0)
    d.sync()
    return dtx.cpu().numpy(), dy.cpu().numpy()


def _oracle_decode(m, t, J):
    o = Oracle(m, t)

    def decode(y):
        res, _, stats, acc = o.kaneko_batch(y, J=J)
        return res, acc != 0, stats
    return decode


def _device_decode(d):
    F = load()

    def decode(y):
        res, _, st = d.decode(y)
        return res, (st["flags"] & F.F_ACCEPTED) != 0, np.stack([st["decodes"], st["comparisons"], st["sums"]], axis=1)
    return decode


def _check_sweep(d, decode, p, e, require_accepted):
    runs = {b: d.sweep_device(p, e, max_snr=SWEEP_MAX_SNR, seed=SWEEP_SEED, batch=b) for b in SWEEP_BATCHES}
    rows = {b: [line.split(",") for line in r[0].strip().splitlines()] for b, r in runs.items()}
    want, cuts, never = _replay_sweep(d, decode, p, e, SWEEP_MAX_SNR, SWEEP_SEED)
    print("BCH(%d,%d) sweep p=%d e=%d:" % (d.n, d.k, p, e), want, cuts, "never accepted:", never)
    if require_accepted:
        assert never == 0
    cols = (0, 1, 3, 4, 5) if never else (0, 1, 2, 3, 4, 5)  # the BER column: include/bchk.h's divergence
    assert [r[0] for r in want] == ["0", "0.5", "1"]
    for b in SWEEP_BATCHES:
        assert len(rows[b]) == len(want), b
        for got, ref in zip(rows[b], want):
            assert [got[c] for c in cols] == [ref[c] for c in cols], (b, got, ref)
    for ref, cut in zip(want, cuts):
        words = e / float(ref[1]) if cut == "errors" else p
        assert words <= p and (cut == "words" or abs(words - round(words)) < 1e-4 * words)
    return cuts


@pytest.mark.gpu
def test_gpu_bch_sweep_matches_word_by_word_replay_15_7():
    """BCH(15,7,5), decoded by the C oracle. At Eb/N0 <= 1 dB the frame error rate is far above
    e / p = 40 / 3000, so every point of the stated run is cut by errors; the second run, with
    p = 200 at the same e, ends its 0 dB point at the 40th error (word 194) and the other two
    after 200 words with 31 and 28 errors (worked out on the CPU from the reference stream and
    the oracle), so both ways of ending a point are replayed. No word of this seed is left
    unaccepted, so the BER column is compared too."""
    d = load().KanekoKernelProcessor(4, 2, J=15)
    cuts = _check_sweep(d, _oracle_decode(4, 2, 15), SWEEP_P, SWEEP_E, True)
    assert cuts == ["errors"] * 3
    cuts = _check_sweep(d, _oracle_decode(4, 2, 15), 200, SWEEP_E, True)
    assert cuts == ["errors", "words", "words"]


@pytest.mark.gpu
def test_gpu_bch_sweep_matches_word_by_word_replay_63_30():
    """BCH(63,30,13): the replay decodes through bchk_decode_variant_host with a stats record
    (the search kernels), a different path from the sweep's fused decode-and-count."""
    d = load().KanekoKernelProcessor(6, 6, J=15)
    cuts = _check_sweep(d, _device_decode(d), SWEEP_P, SWEEP_E, False)
    assert "errors" in cuts, cuts
