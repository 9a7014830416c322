"""The polar simulation front-end over block, correlated and Rician fading (three more
instantiations of polar_gen_kernel in csrc/polar_channel.hip behind the bchk_polar_*_fading*
entry points; FadingChannel for channel= of PolarListDecoder.generate_device / sweep_device /
genie_run and design_genie).

The checker is tests/fading_lib.py, a numpy restatement written from include/bchk.h on top of
philox_lib and channel_lib. Everything here is exact (bytes, bit patterns, integer counters)
except the bounds against the high-precision restatement, derived in
test_gpu_h_against_the_high_precision_restatement, and the statistics, whose standard errors
fading_lib derives.

Shapes, batches and word0 are those of tests/test_polar_channels.py.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import channel_lib as CL
import fading_lib as FL
import philox_lib as P
from bchk_pkg import load
from genie_lib import rank_frozen
from polar_lib import arikan_spec, shorten
from test_polar_channels import (CASE_IDS, CASES, CODES, LENGTHS, SEED, SNR, SPLIT, _high, _sync, _zeros, bits,
                                 decoder, legacy, run as channel_run, sigma_var)

NEW = ("bchk_polar_generate_fading_device", "bchk_polar_sweep_fading_device", "bchk_polar_genie_run_fading",
       "bchk_polar_design_genie_fading", "bchk_polar_sweep_q8_fading_device")
RHOS, KFACTORS = (0.0, 0.9), (0.0, 3.0, 1e6)
# one model of every kind for the checks that do not depend on the parameter
KINDS = (("rayleigh_block", 5), ("rayleigh_correlated", 0.9), ("rician", 3.0))
KIND_IDS = [k for k, _ in KINDS]
STAT_NAME, STAT_B = "short_n7", 65  # 65 x 123 elements


# ---------------------------------------------------------------- host side (no GPU needed)

def test_new_entry_points_are_exported_and_bound():
    F = load()
    lib = F.lib()
    for s in NEW:
        assert s in F.EXPORTS, s
        assert hasattr(lib, s), s
    assert (F.FADING_BLOCK, F.FADING_CORRELATED, F.FADING_RICIAN) == (0, 1, 2)
    assert F.FADINGS == FL.KINDS
    assert F.FadingChannel("rician", 3).param == 3.0


def test_the_channel_names_are_unchanged():
    F = load()
    assert F.CHANNELS == {"awgn": 0, "rayleigh": 1, "bsc": 2}
    assert (F.CHANNEL_AWGN, F.CHANNEL_RAYLEIGH, F.CHANNEL_BSC) == (0, 1, 2)
    d = F.PolarListDecoder.__new__(F.PolarListDecoder)
    d._h, d.U, d.llr = None, 1, "f32"  # no context: the name is checked before the library is called
    for bad in (3, None, "bec", "BSC", "rician", ("rician", 3.0)):
        for call in (lambda: d.generate_device(1.0, 1, 0, channel=bad), lambda: d.sweep_device(1.0, 1.0, 1, 1, 1, channel=bad),
                     lambda: d.genie_run(1.0, 1, channel=bad), lambda: F.design_genie("A A", 2, 1.0, 1, channel=bad)):
            with pytest.raises(ValueError, match="channel"):
                call()


def test_fading_channel_validates_its_parameter():
    F = load()
    nan, inf = float("nan"), float("inf")
    for kind in (0, None, "block", "rayleigh", "RICIAN"):
        with pytest.raises(ValueError, match="kind"):
            F.FadingChannel(kind, 1)
    no_number = ("x", "5", b"5", None, True, False, [5], 5j, np.str_("5"))
    bad = {"rayleigh_block": (0, -1, 0.5, 1.5, nan, inf) + no_number,
           "rayleigh_correlated": (-0.1, 1.0, 1.5, nan, inf) + no_number,
           "rician": (-1.0, -1e-300, nan, inf) + no_number}
    good = {"rayleigh_block": (1, 5, 5.0, 2 ** 40, np.int64(5), np.float32(5)),
            "rayleigh_correlated": (0, 0.0, 0.9, 1 - 2.0 ** -53, np.float64(0.9)),
            "rician": (0, 3.0, 1e6, 1e300, np.float64(3))}
    for kind in FL.KINDS:
        for v in bad[kind]:
            with pytest.raises(ValueError, match=kind):
                F.FadingChannel(kind, v)
        for v in good[kind]:
            ch = F.FadingChannel(kind, v)
            assert (ch.kind, ch.param) == (kind, float(v))


def test_refusals_before_the_context_is_touched():
    """Every BCHK_EINVAL case of (kind, param), through the C ABI with a NULL context: the
    message names the argument; a valid pair gets as far as the context."""
    lib = load().lib()
    host = np.zeros(64, np.float64)
    ptr = host.ctypes.data_as(C.c_void_p)  # never dereferenced: the call is refused first
    nan, inf = float("nan"), float("inf")

    def design(kind, par, K=4):
        buf = C.create_string_buffer(b"untouched", 4096)
        needed = C.c_size_t(12345)
        err, soft = np.full(8, 7, np.uint64), np.full(8, 7, np.int64)
        rc = lib.bchk_polar_design_genie_fading(b"A A A", None, K, kind, par, 1.0, 64, 1, 0, err.ctypes.data_as(C.c_void_p),
                                                soft.ctypes.data_as(C.c_void_p), buf, len(buf), C.byref(needed))
        assert needed.value == 0 and (err == 7).all() and (soft == 7).all() and buf.value == b"untouched"
        return rc

    calls = {
        "generate": lambda k, v: lib.bchk_polar_generate_fading_device(None, k, v, 1.0, 1, 1, 0, None, None, ptr, ptr, None, None),
        "sweep": lambda k, v: lib.bchk_polar_sweep_fading_device(None, k, v, 1.0, 1.0, 1, 10, 1, 1, 0, ptr, None, None),
        "sweep_q8": lambda k, v: lib.bchk_polar_sweep_q8_fading_device(None, k, v, 1.0, 1.0, 1, 10, 1, 1, 0, ptr, None, None, 4.0, 63),
        "genie_run": lambda k, v: lib.bchk_polar_genie_run_fading(None, k, v, 1.0, 10, 1, 0, 0, ptr, ptr, None),
        "design": design,
    }
    cases = [(k, 1.0, "kind") for k in (-1, 3, 77, -(2 ** 31), 2 ** 31 - 1)]
    cases += [(FL.BLOCK, v, "block size") for v in (0.0, -1.0, 0.5, 1.5, 2.0 ** 51 + 0.5, nan, inf, -inf)]
    cases += [(FL.CORRELATED, v, "rho") for v in (-2.0 ** -60, -1.0, 1.0, 1.5, nan, inf)]
    cases += [(FL.RICIAN, v, "K-factor") for v in (-1.0, -2.0 ** -1000, nan, inf, -inf)]
    for name, call in calls.items():
        for kind, v, word in cases:
            assert call(kind, v) == -1, (name, kind, v)
            msg = lib.bchk_last_error().decode()
            assert word in msg, (name, kind, v, msg)
        for kind, v in ((FL.BLOCK, 1.0), (FL.BLOCK, 1e15), (FL.CORRELATED, 0.0), (FL.CORRELATED, 1 - 2.0 ** -53),
                        (FL.RICIAN, 0.0), (FL.RICIAN, 1e300)):
            if name == "design":
                continue  # a valid pair there builds a context
            assert call(kind, v) == -1, (name, kind, v)
            assert "NULL" in lib.bchk_last_error().decode(), (name, kind, v)
    # the plain-channel entry points refuse ids past the BSC as before
    assert lib.bchk_polar_generate_channel_device(None, 3, 1.0, 1, 1, 0, None, None, ptr, None, None, None) == -1
    assert "channel" in lib.bchk_last_error().decode()


def test_restatement_self_checks():
    """The AR(1) recursion is the product with the Cholesky factor of rho^|i-j| (N / 2 = 5), that
    factor is one, and the Rician parameters have 2 s^2 + v^2 = 1 and K = v^2 / (2 s^2)."""
    n = 5
    z, _ = FL.word_pairs(FL.TAG_CORRELATED, n, SEED, 0, 3)
    tol = FL.scalar(2.0 ** -50, None)
    for rho in (0.0, 0.3, 0.9, 1 - 2.0 ** -20):
        Lm = FL.ar1_cholesky(n, rho)
        r = FL.scalar(rho, None)
        cov = Lm.dot(Lm.T)
        for i in range(n):
            for j in range(n):
                assert abs(cov[i, j] - r ** abs(i - j)) <= tol, (rho, i, j)  # c is a rounded double: 2^-52
            assert all(Lm[i, j] == 0 for j in range(i + 1, n))
        g = FL.ar1(z, rho)
        want = np.array([Lm.dot(row) for row in z])
        assert (abs(g - want) <= tol * (1 + abs(want))).all(), rho
    for K in (0.0, 0.5, 3.0, 1e6, 1e300):
        v, s = (float(x) for x in FL.rice_vs(K))
        assert abs(2 * s * s + v * v - 1.0) <= 2.0 ** -50, K
        if 0 < K < 1e100:
            assert abs(v * v / (2 * s * s) / K - 1.0) <= 2.0 ** -49, K
    assert FL.rice_vs(0.0)[0] == 0.0 and float(FL.rice_vs(0.0)[1]) == math.sqrt(0.5)
    # the counters: word, tag, index
    r = P.philox4x32_10((np.array([7], np.uint64), 1, FL.TAG_RICIAN, 4), (SEED, 0))
    z1, z2 = P.normal_from_units_ld(*[P.unit53_int(r[i], r[i + 1]) for i in (0, 2)]) if P.HAVE_LD else \
        P.normal_from_units_dec(int(P.unit53_int(r[0], r[1])[0]), int(P.unit53_int(r[2], r[3])[0]))
    w1, w2 = FL.word_pairs(FL.TAG_RICIAN, 5, SEED, (1 << 32) + 7, 1)
    assert w1[0, 4] == np.ravel(z1)[0] and w2[0, 4] == np.ravel(z2)[0]
    # S = 1 is the i.i.d. factor; a block takes its first element's
    v = CL.word_units(123, SEED, 3, 2)
    np.testing.assert_array_equal(FL.block_units(123, 1, SEED, 3, 2), v)
    np.testing.assert_array_equal(FL.block_units(123, 5, SEED, 3, 2)[:, 119], v[:, 115])
    np.testing.assert_array_equal(FL.block_units(123, 5, SEED, 3, 2)[:, 122], v[:, 120])
    np.testing.assert_array_equal(FL.block_units(123, 200, SEED, 3, 2), np.repeat(v[:, :1], 123, axis=1))


def check_statistics(h_of, lag_of, B=STAT_B):
    """The two statistical assertions on h [B][123] of every model, shared by the restatement
    (CPU) and the device (GPU): h_of(kind, param) and lag_of() = h of rho = 0.9."""
    N = LENGTHS[STAT_NAME]
    for kind, par in [("rayleigh_block", 1), ("rayleigh_block", 5)] + [("rayleigh_correlated", r) for r in RHOS] + \
            [("rician", k) for k in KFACTORS]:
        h = h_of(kind, par)
        assert h.shape == (B, N)
        mean, se = float((h * h).mean()), FL.se_mean_h2(kind, par, N, B)
        print("%s %g: mean h^2 = %.5f, %.2f standard errors from 1" % (kind, par, mean, (mean - 1) / se))
        assert abs(mean - 1.0) < 5 * se, (kind, par)
    h = lag_of()
    hq = h[:, 0::2]
    est, se = FL.lag1_estimate(hq * hq), FL.se_lag1(0.9, hq.shape[1], B)
    print("lag-1 correlation of h_q^2 at rho = 0.9: %.4f, %.2f standard errors from 0.81" % (est, (est - 0.81) / se))
    assert abs(est - 0.81) < 5 * se


def test_the_restatement_passes_the_statistics_with_the_tests_seed():
    """65 words where np.longdouble is wider than a double, the decimal path's few otherwise (the
    standard errors are those of the words used)."""
    N, B = LENGTHS[STAT_NAME], FL.words_of(STAT_B)
    ref = lambda kind, par: FL.to_double(FL.fading(kind, par, N, SEED, 0, B))  # noqa: E731
    check_statistics(ref, lambda: ref("rayleigh_correlated", 0.9), B)


# ---------------------------------------------------------------- GPU helpers

def generate(d, kind, param, B, word0, seed=SEED, want_h=True, want_y=True, snr=SNR):
    """dict(info, cw, llr, h, y) of words [word0, word0 + B) over FadingChannel(kind, param)."""
    import torch
    t_info, t_cw = _zeros((B, d.K), torch.uint8), _zeros((B, d.N), torch.uint8)
    t_llr = _zeros((B, d.N), torch.float32)
    t_h = _zeros((B, d.N), torch.float64) if want_h else None
    t_y = _zeros((B, d.N), torch.float64) if want_y else None
    _sync()
    d.generate_device(snr, B, t_llr.data_ptr(), t_info.data_ptr(), t_cw.data_ptr(), seed=seed, word0=word0,
                      channel=load().FadingChannel(kind, param), d_h=t_h.data_ptr() if want_h else None,
                      d_y=t_y.data_ptr() if want_y else None)
    d.sync()
    return dict(info=t_info.cpu().numpy(), cw=t_cw.cpu().numpy(), llr=t_llr.cpu().numpy(),
                h=t_h.cpu().numpy() if want_h else None, y=t_y.cpu().numpy() if want_y else None)


@functools.lru_cache(maxsize=None)
def run(name, B, word0, kind, param):
    """One device run per (case, model), shared by the tests and left unchanged."""
    return generate(decoder(name), kind, param, B, word0)


def same(a, b, msg=""):
    np.testing.assert_array_equal(a if a.dtype == np.uint8 else bits(a), b if b.dtype == np.uint8 else bits(b), err_msg=msg)


# ---------------------------------------------------------------- 1. the stream, the LLR, the noise

@pytest.mark.gpu
@pytest.mark.parametrize("name,B,word0", CASES, ids=CASE_IDS)
def test_gpu_fading_shares_the_stream(name, B, word0):
    """Information bits and codewords are the AWGN stream's; the LLR is float32(((-2 h) y) /
    sigma^2) of the device's own h and y, bit for bit, with or without d_h and d_y; and y is
    h x + sigma z of the AWGN stream's z, as the Rayleigh test of test_polar_channels.py
    establishes it: with the device's own h (h x is exact), sigma z carries 2^-49 |sigma z_ref| and
    the sum rounds once, at most 2^-52 of the largest of |y|, |sigma z_ref| and h."""
    d, old = decoder(name), legacy(name, B, word0)
    sigma, var = sigma_var(d)
    R = FL.words_of(B)
    noise = P.lift(sigma) * P.element_noise(word0 * d.N, R * d.N, SEED).reshape(R, d.N)
    for kind, par in KINDS:
        got = run(name, B, word0, kind, par)
        same(got["info"], old["info"], kind)
        same(got["cw"], old["cw"], kind)
        same(got["llr"], (-2.0 * got["h"] * got["y"] / var).astype(np.float32), kind)
        assert (got["h"] >= 0).all() and np.isfinite(got["llr"]).all()
        x = np.where(got["cw"][:R] != 0, 1.0, -1.0)
        y_ref = P.lift(got["h"][:R] * x) + noise
        err = abs(P.lift(got["y"][:R]) - y_ref)
        big = np.maximum(np.maximum(abs(y_ref), abs(noise)), P.lift(got["h"][:R]))
        bound = FL.scalar(2.0 ** -49, None) * abs(noise) + FL.scalar(2.0 ** -52, None) * big
        bad = np.argwhere(~(err <= bound))
        assert not len(bad), (kind, bad[:5].tolist())
    if B == 7:  # the optional outputs do not change the others
        kind, par = KINDS[1]
        got = run(name, B, word0, kind, par)
        same(generate(d, kind, par, B, word0, want_h=False, want_y=False)["llr"], got["llr"])
        same(generate(d, kind, par, B, word0, want_h=False)["y"], got["y"])
        same(generate(d, kind, par, B, word0, want_y=False)["h"], got["h"])


# ---------------------------------------------------------------- 2. block fading, exact

@pytest.mark.gpu
@pytest.mark.parametrize("name,B,word0", CASES, ids=CASE_IDS)
def test_gpu_block_fading_is_the_rayleigh_factor_of_the_block(name, B, word0):
    d = decoder(name)
    N = d.N
    ray = channel_run(name, B, word0, "rayleigh")
    one = run(name, B, word0, "rayleigh_block", 1)
    for key in ("llr", "h", "y", "info", "cw"):  # S = 1 is channel="rayleigh" bit for bit
        same(one[key], ray[key], key)
    five = run(name, B, word0, "rayleigh_block", 5)
    first = (np.arange(N) // 5) * 5
    assert N % 5 != 0  # the last block is short
    same(five["h"], ray["h"][:, first])
    h_ref = FL.block_fading(N, 5, SEED, word0, FL.words_of(B))
    assert (abs(P.lift(five["h"][:len(h_ref)]) - h_ref) <= FL.scalar(1.5 * 2.0 ** -52 + 2.0 ** -59, None) * h_ref).all()
    for S in (N, N + 3, 2 ** 40):
        whole = run(name, B, word0, "rayleigh_block", S)
        same(whole["h"], np.repeat(ray["h"][:, :1], N, axis=1), str(S))
    if N > 5:
        assert (five["h"][:, 0] != five["h"][:, 5]).all()


# ---------------------------------------------------------------- 3. correlated fading: the QAM symbols

@pytest.mark.gpu
@pytest.mark.parametrize("name,B,word0", CASES, ids=CASE_IDS)
def test_gpu_correlated_fading_pairs_the_elements(name, B, word0):
    d = decoder(name)
    for rho in RHOS:
        h = run(name, B, word0, "rayleigh_correlated", rho)["h"]
        pairs = d.N // 2
        same(h[:, 0:2 * pairs:2], h[:, 1:2 * pairs:2], str(rho))
        assert (h[:, 0:2 * pairs - 2:2] != h[:, 2:2 * pairs:2]).all()


# ---------------------------------------------------------------- 4. order independence

@pytest.mark.gpu
@pytest.mark.parametrize("kind,par", KINDS + (("rayleigh_block", 200),), ids=KIND_IDS + ["one_block"])
@pytest.mark.parametrize("name,word0", [(n, w) for n in CODES for w in (0, _high(n))],
                         ids=[f"{n}-{t}" for n in CODES for t in ("w0", "high")])
def test_gpu_a_batch_is_its_parts(name, word0, kind, par):
    """65 words give the same bits as the parts 1 + 7 + 57 of the same stream, each part reached
    from its own word0 on its own grid."""
    d = decoder(name)
    whole = run(name, 65, word0, kind, par)
    parts, at = [], word0
    for n in SPLIT:
        parts.append(generate(d, kind, par, n, at))
        at += n
    for key, a in whole.items():
        same(a, np.concatenate([p[key] for p in parts]), key)
    tail = generate(d, kind, par, 5, word0 + 60)  # and the last words alone
    for key, a in whole.items():
        same(a[60:], tail[key], key)


# ---------------------------------------------------------------- 5. h against the restatement

def hyp_bound(a_ref, b_ref, ea, eb, half):
    """The bound on |h - h_ref| for h = sqrt((a^2 + b^2) [/ 2]) formed in doubles from a, b within
    ea, eb of a_ref, b_ref (everything in the reference's number type):
      fl(a^2) = a^2 (1 + d), |d| <= 2^-53, and |a^2 - a_ref^2| <= 2 |a_ref| ea + ea^2, so
        |fl(a^2) - a_ref^2| <= (2 |a_ref| ea + ea^2)(1 + 2^-53) + 2^-53 a_ref^2 =: eA;
      the sum rounds once: |S - S_ref| <= (eA + eB)(1 + 2^-53) + 2^-53 S_ref; halving is exact;
      the square root is within 1 ulp (the figure test_polar_channels.py uses), 2^-52 relative, and
        |sqrt(x) - sqrt(x_ref)| = |x - x_ref| / (sqrt(x) + sqrt(x_ref)) <= |x - x_ref| / h_ref;
      the reference's own error is below 2^-59 relative (test_polar_channels.py)."""
    k = lambda v: FL.scalar(v, None)  # noqa: E731
    up, r53 = k(1 + 2.0 ** -53), k(2.0 ** -53)
    eA = (2 * abs(a_ref) * ea + ea * ea) * up + r53 * a_ref * a_ref
    eB = (2 * abs(b_ref) * eb + eb * eb) * up + r53 * b_ref * b_ref
    s_ref = a_ref * a_ref + b_ref * b_ref
    dx = (eA + eB) * up + r53 * s_ref
    x_ref = s_ref / 2 if half else s_ref
    if half:
        dx = dx / 2
    h_ref = FL.sqrt_ref(x_ref)
    return h_ref, dx / h_ref * k(1 + 2.0 ** -52) + k(2.0 ** -52 + 2.0 ** -59) * h_ref


def term_bound(t_ref):
    """|fl(c z) - c z_ref| for the device's z within 2^-49 relative of z_ref (the device normal's
    bound of tests/test_stream_reference.py) and one rounding of the product: (2^-49 + 2^-53)
    |c z_ref|, with 2^-40 relative for the second-order terms."""
    return FL.scalar((2.0 ** -49 + 2.0 ** -53) * (1 + 2.0 ** -40), None) * abs(t_ref)


def report(tag, err, bound):
    ratio = max(float(e) for e in (err / bound).ravel())
    print("%s: worst |h - h_ref| / bound = %.4f" % (tag, ratio))
    bad = np.argwhere(~(err <= bound))
    assert not len(bad), (tag, bad[:5].tolist())


def check_correlated_h(tag, h, N, rho, word0):
    """h [R][N] of the device against the restatement of words [word0, word0 + R), within the bound
    that test_gpu_h_against_the_high_precision_restatement derives."""
    k = lambda v: FL.scalar(v, None)  # noqa: E731
    a, b, ta, tb = FL.correlated_gauss(N, rho, SEED, word0, len(h))
    amp = k((1 + 2.0 ** -40) / (1.0 - rho))
    ea = amp * (term_bound(ta) + k(2.0 ** -53) * abs(a)).max(axis=1)[:, None]
    eb = amp * (term_bound(tb) + k(2.0 ** -53) * abs(b)).max(axis=1)[:, None]
    h_ref, bound = hyp_bound(a, b, ea, eb, True)
    report(tag, abs(P.lift(h[:, 0::2]) - h_ref), bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,word0", CASES, ids=CASE_IDS)
def test_gpu_h_against_the_high_precision_restatement(name, B, word0):
    """d_h of the correlated (rho = 0, 0.9) and Rician (K = 0, 3, 10^6) models against fading_lib.

    Correlated: the device forms t_q = fl(c z_q) (t_0 = z_0) and g_q = fma(rho, g_{q-1}, t_q) =
    (rho g_{q-1} + t_q)(1 + d), |d| <= 2^-53, from the same doubles rho and c as the restatement. With
    e_q = |g_q - G_q| and term_bound: e_q <= rho e_{q-1} + term_bound(T_q) + 2^-53 (|G_q| + e_q). The
    recursion is a contraction, so along a word e_q <= max_q (term_bound(T_q) + 2^-53 |G_q|) / (1 - rho),
    again with 2^-40 relative for the second-order term. hyp_bound carries that to h.
    Rician: re = fl(v + fl(s z1)): |re - re_ref| <= term_bound(s z1) + 2^-53 (|re_ref| + term_bound);
    im = fl(s z2): term_bound(s z2); then hyp_bound without the halving.
    At K = 10^6: |h - 1| <= (1 - v) + s sqrt(z1^2 + z2^2) by the triangle inequality, and the radius
    sqrt(-2 log u1) of a Box-Muller pair is at most sqrt(106 log 2) < 8.58 (u1 >= 2^-53)."""
    d = decoder(name)
    N, R = d.N, FL.words_of(B)
    k = lambda v: FL.scalar(v, None)  # noqa: E731
    for rho in RHOS:
        check_correlated_h("%s rho = %g" % (name, rho), run(name, B, word0, "rayleigh_correlated", rho)["h"][:R], N, rho, word0)
    for K in KFACTORS:
        got = run(name, B, word0, "rician", K)["h"][:R]
        re, im, t1 = FL.rician_parts(N, K, SEED, word0, R)
        e1 = term_bound(t1)
        h_ref, bound = hyp_bound(re, im, e1 + k(2.0 ** -53) * (abs(re) + e1), term_bound(im), False)
        report("%s K = %g" % (name, K), abs(P.lift(got) - h_ref), bound)
        if K == 1e6:
            v, s = (float(x) for x in FL.rice_vs(K))
            assert np.abs(got - 1.0).max() <= (1.0 - v) + math.sqrt(106 * math.log(2)) * s
            assert np.abs(got - 1.0).max() > 0


# ---------------------------------------------------------------- 5b. the recursion across chunks

# The correlated kernel goes in chunks of 64 QAM symbols and carries g from one chunk to the next.
# The shapes above have at most 62 symbols; these have several chunks: N = 256 is two full ones
# (symbol 64 is lane 0 of a chunk, scaled by c where symbol 0 is not), N = 507 (odd: the last
# symbol half filled, pairs straddling words) is three full ones and a tail of 62.
LONG = {
    "a256": lambda: arikan_spec(8, 128),
    "short_n9": lambda: shorten(lambda **kw: arikan_spec(9, 200, dyn=4, seed=9, **kw), 512, 3, (1, 300)),
}
LONG_N = {"a256": 256, "short_n9": 507}
LONG_CASES = [(n, B, w) for n in LONG for B, w in ((7, 0), (65, (1 << 32) // LONG_N[n] - 30))]


@functools.lru_cache(maxsize=None)
def long_decoder(name):
    d = load().PolarListDecoder(LONG[name](), 1)
    assert d.N == LONG_N[name]
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,word0", LONG_CASES, ids=[f"{n}-B{B}-{'w0' if w == 0 else 'high'}" for n, B, w in LONG_CASES])
def test_gpu_correlated_fading_across_chunks(name, B, word0):
    """More than 64 QAM symbols a word: h against the high-precision restatement (rho = 0 and 0.9,
    the bound of test_gpu_h_against_the_high_precision_restatement), h[2q] == h[2q+1], the LLR
    from the device's own h and y, the AWGN stream's bits, and a batch equal to its parts."""
    d = long_decoder(name)
    N, R = d.N, FL.words_of(B)
    assert (N + 1) // 2 > 64
    _, var = sigma_var(d)
    awgn = generate_awgn(d, B, word0)
    for rho in RHOS:
        got = generate(d, "rayleigh_correlated", rho, B, word0)
        check_correlated_h("%s rho = %g" % (name, rho), got["h"][:R], N, rho, word0)
        pairs = N // 2
        same(got["h"][:, 0:2 * pairs:2], got["h"][:, 1:2 * pairs:2], str(rho))
        assert (got["h"][:, 0:2 * pairs - 2:2] != got["h"][:, 2:2 * pairs:2]).all()
        same(got["llr"], (-2.0 * got["h"] * got["y"] / var).astype(np.float32), str(rho))
        same(got["info"], awgn["info"])
        same(got["cw"], awgn["cw"])
        sizes = SPLIT if B == 65 else (1, 2, 4)
        parts, at = [], word0
        for n in sizes:
            parts.append(generate(d, "rayleigh_correlated", rho, n, at))
            at += n
        for key, a in got.items():
            same(a, np.concatenate([p[key] for p in parts]), key)


def generate_awgn(d, B, word0):
    import torch
    t_info, t_cw = _zeros((B, d.K), torch.uint8), _zeros((B, d.N), torch.uint8)
    t_llr = _zeros((B, d.N), torch.float32)
    _sync()
    d.generate_device(SNR, B, t_llr.data_ptr(), t_info.data_ptr(), t_cw.data_ptr(), seed=SEED, word0=word0)
    d.sync()
    return dict(info=t_info.cpu().numpy(), cw=t_cw.cpu().numpy())


# ---------------------------------------------------------------- 6. statistics

@pytest.mark.gpu
def test_gpu_fading_statistics():
    """Over 65 x 123 elements: the mean of h^2 within five standard errors of 1 for every model,
    and for rho = 0.9 the lag-1 correlation of h_q^2 within five of rho^2 (fading_lib derives both
    standard errors; test_the_restatement_passes_the_statistics_with_the_tests_seed is the same
    check of the restatement alone)."""
    check_statistics(lambda kind, par: run(STAT_NAME, STAT_B, 0, kind, par)["h"],
                     lambda: run(STAT_NAME, STAT_B, 0, "rayleigh_correlated", 0.9)["h"])


# ---------------------------------------------------------------- 7. sweep

SW_POINTS, SW_WORDS, SW_ERRORS, SW_SEED, SW_CHUNK = 3, 4000, 3, 11, 50
SW_FROM, SW_STEP = 0.0, 1.0
Q8_SCALE, Q8_QMAX = 4.0, 63


def loop_sweep(d, chan):
    """generate -> (quantize) -> decode -> count in chunks over the same word indices, the cut
    applied in word order from the per-word flags, the prefix counted again.
    -> (records, first word of every point, whether the last counted word of each is an error)."""
    import torch
    q8 = d.llr == "q8"
    recs, starts, ends_on_error, word = [], [], [], 0
    for pt in range(SW_POINTS):
        par = SW_FROM + pt * SW_STEP
        c = np.zeros(8, np.int64)
        starts.append(word)
        last = False
        while c[0] < SW_WORDS and c[1] < SW_ERRORS:
            nb = int(min(SW_CHUNK, SW_WORDS - c[0]))
            info_tx, cw_tx = _zeros((nb, d.K), torch.uint8), _zeros((nb, d.N), torch.uint8)
            llr, llr8 = _zeros((nb, d.N), torch.float32), _zeros((nb, d.N), torch.int8)
            info, cw = _zeros((nb, d.L, d.K), torch.uint8), _zeros((nb, d.L, d.N), torch.uint8)
            met, cnt = _zeros((nb, d.L), torch.float32), _zeros((nb,), torch.int32)
            flags, out8 = _zeros((nb,), torch.uint8), _zeros((8,), torch.int64)
            _sync()
            d.generate_device(par, nb, llr.data_ptr(), info_tx.data_ptr(), cw_tx.data_ptr(), seed=SW_SEED, word0=word,
                              channel=chan)
            if q8:
                d.quantize_device(llr.data_ptr(), nb * d.N, llr8.data_ptr(), Q8_SCALE, Q8_QMAX)
            d.decode_device((llr8 if q8 else llr).data_ptr(), nb, info.data_ptr(), cw.data_ptr(), met.data_ptr(),
                            cnt.data_ptr())
            d.count_device(info_tx.data_ptr(), cw_tx.data_ptr(), llr.data_ptr(), info.data_ptr(), cw.data_ptr(),
                           cnt.data_ptr(), nb, out8.data_ptr(), flags.data_ptr())
            d.sync()
            fl = flags.cpu().numpy()
            errs = np.flatnonzero(fl & 1)
            need = SW_ERRORS - int(c[1])
            used = nb if len(errs) < need else int(errs[need - 1]) + 1
            if used < nb:
                out8.zero_()
                _sync()
                d.count_device(info_tx.data_ptr(), cw_tx.data_ptr(), llr.data_ptr(), info.data_ptr(), cw.data_ptr(),
                               cnt.data_ptr(), used, out8.data_ptr())
                d.sync()
            c += out8.cpu().numpy()
            word += used
            last = bool(fl[used - 1] & 1)
        recs.append((par, [int(v) for v in c]))
        ends_on_error.append(last)
    return recs, starts, ends_on_error


@functools.lru_cache(maxsize=None)
def sweep_decoder(llr):
    return load().PolarListDecoder(CODES["a8k4"](), 2, llr=llr)


@pytest.mark.gpu
@pytest.mark.parametrize("llr", ["f32", "q8"])
@pytest.mark.parametrize("kind,par", KINDS, ids=KIND_IDS)
def test_gpu_fading_sweep_matches_the_loop(kind, par, llr):
    """(8, 4), L = 2, three points, every one cut at its third block error: all eight counters of
    sweep_device equal the Python loop's at batch 7 and 0, on the f32 and the int8 decoder."""
    F = load()
    d = sweep_decoder(llr)
    chan = F.FadingChannel(kind, par)
    extra = dict(scale=Q8_SCALE, qmax=Q8_QMAX) if llr == "q8" else {}
    runs = {b: d.sweep_device(SW_FROM, SW_STEP, SW_POINTS, SW_WORDS, SW_ERRORS, seed=SW_SEED, batch=b, channel=chan,
                              **extra) for b in (7, 0)}
    recs = runs[7][0]
    print(kind, llr, "sweep:", recs)
    assert runs[0][0] == recs
    want, starts, ends_on_error = loop_sweep(d, chan)
    assert recs == want
    assert [r[0] for r in recs] == [SW_FROM + i * SW_STEP for i in range(SW_POINTS)]
    start = 0
    for (_, c), s0, last in zip(recs, starts, ends_on_error):
        assert c[1] == SW_ERRORS and c[0] < SW_WORDS and s0 == start and last  # cut at the last block error
        start += c[0]
    for _, secs, words in runs.values():
        assert secs > 0 and words >= start
    # another model, other words: the parameter reaches the kernel
    other = F.FadingChannel(kind, {"rayleigh_block": 1, "rayleigh_correlated": 0.0, "rician": 0.0}[kind])
    assert d.sweep_device(SW_FROM, SW_STEP, SW_POINTS, SW_WORDS, SW_ERRORS, seed=SW_SEED, batch=0, channel=other,
                          **extra)[0] != recs


# ---------------------------------------------------------------- 8. genie and design

@pytest.mark.gpu
@pytest.mark.parametrize("kind,par", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", ["short_n7", "G_A3"])
def test_gpu_genie_run_is_generate_plus_genie_device(name, kind, par):
    import torch
    d = decoder(name)
    chan = load().FadingChannel(kind, par)
    W, w0 = 100, 37
    e_sum, s_sum, at = np.zeros(d.U, np.int64), np.zeros(d.U, np.int64), w0
    for n in (1, 42, 57):  # generate_device batches, summed
        info, llr = _zeros((n, d.K), torch.uint8), _zeros((n, d.N), torch.float32)
        err, soft = _zeros((d.U,), torch.int64), _zeros((d.U,), torch.int64)
        _sync()
        d.generate_device(SNR, n, llr.data_ptr(), info.data_ptr(), seed=SEED, word0=at, channel=chan)
        d.genie_device(info.data_ptr(), llr.data_ptr(), n, err.data_ptr(), soft.data_ptr())
        d.sync()
        e_sum, s_sum, at = e_sum + err.cpu().numpy(), s_sum + soft.cpu().numpy(), at + n
    assert e_sum.sum() > 0
    for batch in (0, 9):
        e, s, _ = d.genie_run(SNR, W, seed=SEED, word0=w0, batch=batch, channel=chan)
        np.testing.assert_array_equal(e.view(np.int64), e_sum)
        np.testing.assert_array_equal(s, s_sum)
    assert (d.genie_run(SNR, W, seed=SEED, word0=w0, channel="rayleigh")[1] != s_sum).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,par", KINDS, ids=KIND_IDS)
def test_gpu_design_genie_over_a_fading_model(kind, par):
    """A^5, K = 16 at 2 dB: the frozen set is rank_frozen of the counts, and the counts are
    genie_run's over the lowest-indices-frozen code."""
    F = load()
    chan = F.FadingChannel(kind, par)
    layers, K, snr, words = ("A",) * 5, 16, 2.0, 500
    spec, err, soft = F.design_genie(layers, K, snr, words, seed=4, channel=chan)
    lines = spec.strip().split("\n")
    assert lines[0] == "32 16 0 5 0 0" and lines[1] == "A A A A A"
    frozen = [int(ln.split()[1]) for ln in lines[2:]]
    assert all(ln.startswith("1 ") for ln in lines[2:]) and len(set(frozen)) == 32 - K
    assert frozen == rank_frozen(err, soft, K)
    base = "\n".join(lines[:2]) + "\n" + "".join(f"1 {f}\n" for f in range(32 - K))
    e, s, _ = F.PolarListDecoder(base, 1).genie_run(snr, words, seed=4, channel=chan)
    np.testing.assert_array_equal(e, err)
    np.testing.assert_array_equal(s, soft)
    assert err.sum() > 0 and (F.design_genie(layers, K, snr, words, seed=4)[1] != err).any()  # not the AWGN counters


# ---------------------------------------------------------------- 9. refusals that need a context

@pytest.mark.gpu
def test_gpu_dimension_zero_is_refused_on_every_model():
    import torch
    F = load()
    d = F.PolarListDecoder(arikan_spec(4, 0), 2)
    t = _zeros((64,), torch.float64)
    for kind, par in KINDS:
        chan = F.FadingChannel(kind, par)
        with pytest.raises(F.BchkError, match="dimension 0"):
            d.generate_device(SNR, 2, t.data_ptr(), channel=chan)
        with pytest.raises(F.BchkError, match="dimension 0"):
            d.sweep_device(SNR, 0.0, 1, 10, 1, channel=chan)
        with pytest.raises(F.BchkError, match="dimension 0"):
            d.genie_run(SNR, 4, channel=chan)
        decoder("a8k4").generate_device(SNR, 0, None, channel=chan)  # B = 0 is a no-op
    _sync()
    assert not t.cpu().numpy().any()
