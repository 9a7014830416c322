"""The polar simulation front-end over Rayleigh fading and the BSC (csrc/polar_channel.hip behind
bchk_polar_generate_channel_device, bchk_polar_sweep_channel_device, bchk_polar_genie_run_channel,
bchk_polar_design_genie_channel; PolarListDecoder.generate_device / sweep_device / genie_run and
design_genie with channel=).

The checker of the new draw is tests/channel_lib.py, a numpy restatement of u(G) written from
the comments of csrc/bchk_philox.h and include/bchk.h on top of tests/philox_lib.py. Everything
here is exact (bytes, float32 / float64 bit patterns, integer counters) except the two Rayleigh
bounds against the high-precision reference, which are derived in
test_gpu_rayleigh_against_the_high_precision_reference.

Shapes: the smallest where the indexing can go wrong -- all-Arikan (8, 4); the punctured and
shortened Arikan code arikan_n7 of tests/short_codes.py (U = 128, N = 123: odd, so the element
pairs straddle the words); G x A^3 (N = 24, no power of two) -- at batches 1, 7 and 65 (one wave,
two workgroups of 4 waves, 17 workgroups with a partial last one) from word 0, and 65 words from a
word0 that puts the crossing of G = w N + position over 2^32 inside the batch.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import channel_lib as CL
import philox_lib as P
from bchk_pkg import load
from genie_lib import rank_frozen
from polar_lib import arikan_spec
from short_codes import short_spec
from test_polar_mixed_tiered import any_spec

NEW = ("bchk_polar_generate_channel_device", "bchk_polar_sweep_channel_device", "bchk_polar_genie_run_channel",
       "bchk_polar_design_genie_channel")
SEED, SNR = 5, 1.0
BSC_P = (0.5, 0.11, 2.0 ** -53)
CODES = {
    "a8k4": lambda: arikan_spec(3, 4),
    "short_n7": lambda: short_spec("arikan_n7", None),
    "G_A3": lambda: any_spec(("G", "A", "A", "A"), 12, seed=2),
}
LENGTHS = {"a8k4": 8, "short_n7": 123, "G_A3": 24}


def _high(name):
    """A word0 whose 65 words cross G = 2^32."""
    return (1 << 32) // LENGTHS[name] - 30


CASES = [(name, B, 0) for name in CODES for B in (1, 7, 65)] + [(name, 65, _high(name)) for name in CODES]
CASE_IDS = [f"{n}-B{B}-{'w0' if w == 0 else 'high'}" for n, B, w in CASES]
SPLIT = (1, 7, 57)  # the parts of a batch of 65


# ---------------------------------------------------------------- host side (no GPU needed)

def test_new_entry_points_are_exported_and_bound():
    F = load()
    lib = F.lib()
    for s in NEW:
        assert s in F.EXPORTS, s
        assert hasattr(lib, s), s
    assert (F.CHANNEL_AWGN, F.CHANNEL_RAYLEIGH, F.CHANNEL_BSC) == (0, 1, 2)
    assert F.CHANNELS == CL.CHANNELS
    d = F.PolarListDecoder.__new__(F.PolarListDecoder)
    d._h, d.U = None, 1  # no context: the name is checked before the library is called
    for call in (lambda: d.generate_device(1.0, 1, 0, channel="bec"), lambda: d.sweep_device(1.0, 1.0, 1, 1, 1, channel=3),
                 lambda: d.genie_run(1.0, 1, channel=None), lambda: F.design_genie("A A", 2, 1.0, 1, channel="BSC")):
        with pytest.raises(ValueError, match="channel"):
            call()


def test_uniform_restatement_edges():
    """The counter of u(G) is the element pair's, the tag its own; the forced units: v = 2^53 is
    u = 1 (h = 0, never flipped), v = 1 is the smallest unit (the largest h, the only one a BSC of
    p = 2^-53 flips)."""
    r = P.philox4x32_10((np.array([3], np.uint64), 0, CL.TAG_UNIFORM, 0), (SEED, 0))
    v = CL.element_units(6, 3, SEED)  # elements 6, 7 of pair 3 and element 8 of pair 4
    assert int(v[0]) == int(P.unit53_int(r[0], r[1])[0]) and int(v[1]) == int(P.unit53_int(r[2], r[3])[0])
    np.testing.assert_array_equal(CL.element_units(7, 2, SEED), v[1:])
    hi = (1 << 33) + 5  # the pair index needs its high counter word
    r = P.philox4x32_10((np.array([(hi >> 1) & 0xFFFFFFFF], np.uint64), hi >> 33, CL.TAG_UNIFORM, 0), (SEED, 0))
    assert int(CL.element_units(hi, 1, SEED)[0]) == int(P.unit53_int(r[2], r[3])[0])
    forced = np.array([1, 2, 1 << 52, (1 << 53) - 1, 1 << 53], np.uint64)
    assert CL.bsc_flips(forced, 2.0 ** -53).tolist() == [True, False, False, False, False]
    assert CL.bsc_flips(forced, 0.5).tolist() == [True, True, True, False, False]
    for ld in ([True, False] if P.HAVE_LD else [False]):
        h = CL.fading_from_units(forced, ld)
        assert float(h[4]) == 0.0 and abs(float(h[0]) - math.sqrt(53 * math.log(2))) < 1e-14
        assert abs(float(h[2]) - math.sqrt(math.log(2))) < 1e-15
    big = CL.element_units(0, 1 << 16, SEED).astype(np.float64) * 2.0 ** -53
    assert 0 < big.min() and big.max() <= 1.0 and abs(big.mean() - 0.5) < 5 / math.sqrt(12 * len(big))
    if P.HAVE_LD:  # E[h^2] = E[-log u] = 1
        h = CL.fading_from_units(CL.element_units(0, 1 << 16, SEED)).astype(np.float64)
        assert abs((h * h).mean() - 1.0) < 5 / math.sqrt(len(h))


def test_refusals_before_any_device_call():
    """Every BCHK_EINVAL case of include/bchk.h that needs no context, through the C ABI with a
    NULL context: (channel, param) and d_h are checked first, so the message names the argument.
    (K = 0 of a context: test_gpu_dimension_zero_is_refused_on_every_channel.)"""
    F = load()
    lib = F.lib()
    host = np.zeros(64, np.float64)
    ptr = host.ctypes.data_as(C.c_void_p)  # never dereferenced: the call is refused first

    def refused(rc, word):
        assert rc == -1
        msg = lib.bchk_last_error().decode()
        assert word in msg, msg

    bad_p = (0.0, -0.25, 0.5000000000000001, 1.0, float("nan"), float("inf"))
    for ch in (-1, 3, 77):
        refused(lib.bchk_polar_generate_channel_device(None, ch, 1.0, 1, 1, 0, None, None, ptr, None, None, None), "channel")
        refused(lib.bchk_polar_genie_run_channel(None, ch, 1.0, 10, 1, 0, 0, ptr, ptr, None), "channel")
        refused(lib.bchk_polar_sweep_channel_device(None, ch, 1.0, 1.0, 1, 10, 1, 1, 0, ptr, None, None), "channel")
    for p in bad_p:
        refused(lib.bchk_polar_generate_channel_device(None, CL.BSC, p, 1, 1, 0, None, None, ptr, None, None, None), "p =")
        refused(lib.bchk_polar_genie_run_channel(None, CL.BSC, p, 10, 1, 0, 0, ptr, ptr, None), "p =")
        refused(lib.bchk_polar_sweep_channel_device(None, CL.BSC, p, 0.0, 1, 10, 1, 1, 0, ptr, None, None), "p =")
    # a later point of a sweep outside the range: 0.4, 0.5, 0.6
    refused(lib.bchk_polar_sweep_channel_device(None, CL.BSC, 0.4, 0.1, 3, 10, 1, 1, 0, ptr, None, None), "p =")
    for ch in (CL.AWGN, CL.BSC):
        refused(lib.bchk_polar_generate_channel_device(None, ch, 0.25, 1, 1, 0, None, None, ptr, ptr, None, None), "d_h")
    # a valid (channel, param) gets as far as the context
    for ch, par in ((CL.AWGN, -3.0), (CL.RAYLEIGH, 200.0), (CL.BSC, 0.5), (CL.BSC, 2.0 ** -53)):
        refused(lib.bchk_polar_generate_channel_device(None, ch, par, 1, 1, 0, None, None, ptr, None, None, None), "NULL")

    def design(ch, par, K=4):
        buf = C.create_string_buffer(b"untouched", 4096)
        needed = C.c_size_t(12345)
        err, soft = np.full(8, 7, np.uint64), np.full(8, 7, np.int64)
        rc = lib.bchk_polar_design_genie_channel(b"A A A", None, K, ch, par, 64, 1, 0, err.ctypes.data_as(C.c_void_p),
                                                 soft.ctypes.data_as(C.c_void_p), buf, len(buf), C.byref(needed))
        assert needed.value == 0 and (err == 7).all() and (soft == 7).all() and buf.value == b"untouched"
        return rc

    refused(design(5, 1.0), "channel")
    for p in bad_p:
        refused(design(CL.BSC, p), "p =")
    for ch, par in ((CL.RAYLEIGH, 1.0), (CL.BSC, 0.1)):
        refused(design(ch, par, K=0), "dimension")
        refused(design(ch, par, K=9), "dimension")


# ---------------------------------------------------------------- GPU helpers

def _zeros(shape, dtype):
    import torch
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()


_dec = {}


def decoder(name, L=1):
    if (name, L) not in _dec:
        _dec[name, L] = load().PolarListDecoder(CODES[name](), L)
        assert _dec[name, L].N == LENGTHS[name]
    return _dec[name, L]


def param_of(channel, p=0.11):
    return p if channel == "bsc" else SNR


def generate(d, channel, param, B, word0, seed=SEED, want_h=True, want_y=True, legacy=False):
    """dict(info, cw, llr, h, y) of words [word0, word0 + B) as numpy arrays; legacy: through
    bchk_polar_generate_device itself."""
    import torch
    t_info, t_cw = _zeros((B, d.K), torch.uint8), _zeros((B, d.N), torch.uint8)
    t_llr = _zeros((B, d.N), torch.float32)
    t_h = _zeros((B, d.N), torch.float64) if want_h and channel == "rayleigh" and not legacy else None
    t_y = _zeros((B, d.N), torch.float64) if want_y and not legacy else None
    _sync()
    if legacy:
        rc = load().lib().bchk_polar_generate_device(d.handle, param, B, seed, word0, t_info.data_ptr(), t_cw.data_ptr(),
                                                     t_llr.data_ptr(), None)
        assert rc == 0
    else:
        d.generate_device(param, B, t_llr.data_ptr(), t_info.data_ptr(), t_cw.data_ptr(), seed=seed, word0=word0,
                          channel=channel, d_h=t_h.data_ptr() if t_h is not None else None,
                          d_y=t_y.data_ptr() if t_y is not None else None)
    d.sync()
    return dict(info=t_info.cpu().numpy(), cw=t_cw.cpu().numpy(), llr=t_llr.cpu().numpy(),
                h=None if t_h is None else t_h.cpu().numpy(), y=None if t_y is None else t_y.cpu().numpy())


@functools.lru_cache(maxsize=None)
def run(name, B, word0, channel, p=0.11):
    """One device run per (case, channel, p), shared by the tests and left unchanged."""
    return generate(decoder(name), channel, param_of(channel, p), B, word0)


@functools.lru_cache(maxsize=None)
def legacy(name, B, word0):
    return generate(decoder(name), "awgn", SNR, B, word0, legacy=True)


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def sigma_var(d):
    s = np.float64(P.polar_sigma(d.N, d.K, SNR))
    return s, s * s


# ---------------------------------------------------------------- 1. the channels share the stream

@pytest.mark.gpu
@pytest.mark.parametrize("name,B,word0", CASES, ids=CASE_IDS)
def test_gpu_channels_share_the_stream(name, B, word0):
    """d_info and d_cw of every channel are bchk_polar_generate_device's byte for byte; the AWGN
    channel gives its LLRs bit for bit, and d_y is the double they were rounded from."""
    d, old = decoder(name), legacy(name, B, word0)
    np.testing.assert_array_equal(old["info"], P.polar_info(d.K, SEED, word0, B))
    for channel in CL.CHANNELS:
        got = run(name, B, word0, channel)
        np.testing.assert_array_equal(got["info"], old["info"], err_msg=channel)
        np.testing.assert_array_equal(got["cw"], old["cw"], err_msg=channel)
    awgn = run(name, B, word0, "awgn")
    np.testing.assert_array_equal(bits(awgn["llr"]), bits(old["llr"]))
    _, var = sigma_var(d)
    np.testing.assert_array_equal(bits((-2.0 * awgn["y"] / var).astype(np.float32)), bits(old["llr"]))


# ---------------------------------------------------------------- 2. BSC, bit for bit

@pytest.mark.gpu
@pytest.mark.parametrize("name,B,word0", CASES, ids=CASE_IDS)
def test_gpu_bsc_flips_are_the_restated_draws(name, B, word0):
    """The flips are exactly u(G) <= p, the LLRs exactly +-2.0f and d_y exactly +-1. At p = 2^-53
    only a draw of the smallest unit flips; the ABI has no hook that forces a draw (the forced
    units are in test_uniform_restatement_edges), so there the batch must come out unflipped."""
    d = decoder(name)
    v = CL.word_units(d.N, SEED, word0, B)
    for p in BSC_P:
        got = run(name, B, word0, "bsc", p)
        flips = CL.bsc_flips(v, p)
        x = np.where(got["cw"] != 0, 1.0, -1.0)
        y = np.where(flips, -x, x)
        np.testing.assert_array_equal(bits(got["y"]), bits(y), err_msg=str(p))
        np.testing.assert_array_equal(bits(got["llr"]), bits((-2.0 * y).astype(np.float32)), err_msg=str(p))
        assert set(np.unique(got["llr"]).tolist()) <= {-2.0, 2.0}
        if p == 2.0 ** -53:
            assert not flips.any()
            np.testing.assert_array_equal(got["llr"], (-2.0 * x).astype(np.float32))
        elif B * d.N >= 56:  # 5 standard errors of the flip count
            assert abs(flips.mean() - p) < 5 * math.sqrt(p * (1 - p) / flips.size)


# ---------------------------------------------------------------- 3. Rayleigh

@pytest.mark.gpu
@pytest.mark.parametrize("name,B,word0", CASES, ids=CASE_IDS)
def test_gpu_rayleigh_against_the_high_precision_reference(name, B, word0):
    """d_h against sqrt(-log u), d_y against h_ref x + sigma z_ref, both evaluated above double
    (channel_lib / philox_lib: np.longdouble pinned to a 50-digit decimal evaluation within 2^-60,
    or that evaluation itself).

    The bounds, from the double-precision errors the HIP math documentation states for the device
    library (the figures tests/test_stream_reference.py uses: log <= 1 ulp, sqrt <= 1 ulp, and for
    z about 4 * 2^-52 relative, asserted there as 2^-49); 1 ulp is at most 2^-52 relative:
      L' = -log u is L (1 + e1), |e1| <= 2^-52 (the negation is exact, u is exact);
      h = sqrt(L') (1 + e2), |e2| <= 2^-52, is sqrt(L) (1 + e1)^(1/2) (1 + e2): the square root
        halves the logarithm's error and adds its own, 1.5 * 2^-52 relative to first order; the
        second-order terms are below 2^-104 and the reference's own error below 2^-60, so
        |d_h - h_ref| <= (1.5 * 2^-52 + 2^-59) h_ref;
      y = fl(h x + fl(sigma z)): h x is exact (x = +-1), sigma z carries the stream test's bound
        2^-49 |sigma z_ref| (it includes the product's rounding), the sum rounds once, at most
        2^-53 of a result no larger than twice the largest of |y_ref|, |sigma z_ref| and h_ref, so
        |d_y - y_ref| <= bound(h) + 2^-49 |sigma z_ref| + 2^-52 max(|y_ref|, |sigma z_ref|, h_ref).
    The LLR is then checked bit for bit from the device's own h and y: ((-2 h) y) / sigma^2 has
    two products and a division, one rounding each, and nothing to fuse. With d_h and d_y NULL
    the LLRs are the same bits."""
    d = decoder(name)
    got = run(name, B, word0, "rayleigh")
    h_ref, y_ref, noise = CL.rayleigh_words(got["cw"], d.N, d.K, SNR, SEED, word0)
    R = len(h_ref)
    assert R == B or not P.HAVE_LD
    lift = lambda v: P.lift(np.float64(v))  # noqa: E731
    err_h = abs(P.lift(got["h"][:R]) - h_ref)
    bound_h = lift(1.5 * 2.0 ** -52 + 2.0 ** -59) * h_ref
    nz = h_ref != 0
    print("%s: max |h - h_ref| / (2^-52 h_ref) = %.3f over %d elements"
          % (name, max(float(e) for e in (err_h[nz] / (lift(2.0 ** -52) * h_ref[nz])).ravel()), int(nz.sum())))
    bad = np.argwhere(~(err_h <= bound_h))
    assert not len(bad), (bad[:5].tolist(), [float(err_h[tuple(i)]) for i in bad[:5]])
    err_y = abs(P.lift(got["y"][:R]) - y_ref)
    bound_y = bound_h + lift(2.0 ** -49) * abs(noise) + lift(2.0 ** -52) * np.maximum(np.maximum(abs(y_ref), abs(noise)), h_ref)
    bad = np.argwhere(~(err_y <= bound_y))
    assert not len(bad), (bad[:5].tolist(), [float(err_y[tuple(i)]) for i in bad[:5]])
    _, var = sigma_var(d)
    want = (-2.0 * got["h"] * got["y"] / var).astype(np.float32)
    np.testing.assert_array_equal(bits(got["llr"]), bits(want))
    bare = generate(d, "rayleigh", SNR, B, word0, want_h=False, want_y=False)
    np.testing.assert_array_equal(bits(bare["llr"]), bits(got["llr"]))
    only_y = generate(d, "rayleigh", SNR, B, word0, want_h=False)
    np.testing.assert_array_equal(bits(only_y["y"]), bits(got["y"]))
    assert (got["h"] >= 0).all() and (got["llr"] != old_awgn_llr(name, B, word0)).any()


def old_awgn_llr(name, B, word0):
    return legacy(name, B, word0)["llr"]


# ---------------------------------------------------------------- 4. order independence

@pytest.mark.gpu
@pytest.mark.parametrize("channel", list(CL.CHANNELS))
@pytest.mark.parametrize("name,word0", [(n, w) for n in CODES for w in (0, _high(n))],
                         ids=[f"{n}-{t}" for n in CODES for t in ("w0", "high")])
def test_gpu_a_batch_is_its_parts(name, word0, channel):
    """65 words give the same bits as the parts 1 + 7 + 57 of the same stream."""
    d = decoder(name)
    whole = run(name, 65, word0, channel)
    parts, at = [], word0
    for n in SPLIT:
        parts.append(generate(d, channel, param_of(channel), n, at))
        at += n
    for key, a in whole.items():
        if a is None:
            assert all(p[key] is None for p in parts)
            continue
        joined = np.concatenate([p[key] for p in parts])
        np.testing.assert_array_equal(a if a.dtype == np.uint8 else bits(a),
                                      joined if a.dtype == np.uint8 else bits(joined), err_msg=key)


# ---------------------------------------------------------------- 5. sweep

SW_POINTS, SW_WORDS, SW_ERRORS, SW_SEED, SW_CHUNK = 3, 4000, 3, 11, 50
SW_RANGE = {"bsc": (0.05, 0.05), "rayleigh": (0.0, 1.0)}


def raw_sweep(fn, d, *args):
    F = load()
    out = np.zeros(SW_POINTS, F.POLAR_POINT_DTYPE)
    assert fn(d.handle, *args, out.ctypes.data_as(C.c_void_p), None, None) == 0
    return [(float(r["snr_db"]), [int(v) for v in r["c"]]) for r in out]


def loop_sweep(d, channel, frm, step):
    """generate_channel -> decode_device -> count_device in chunks, the cut applied in word order
    from the per-word flags, the prefix counted again. -> (records, first word of every point)."""
    import torch
    recs, starts, word = [], [], 0
    for pt in range(SW_POINTS):
        par = frm + pt * step
        c = np.zeros(8, np.int64)
        starts.append(word)
        while c[0] < SW_WORDS and c[1] < SW_ERRORS:
            nb = int(min(SW_CHUNK, SW_WORDS - c[0]))
            info_tx, cw_tx = _zeros((nb, d.K), torch.uint8), _zeros((nb, d.N), torch.uint8)
            llr = _zeros((nb, d.N), torch.float32)
            info, cw = _zeros((nb, d.L, d.K), torch.uint8), _zeros((nb, d.L, d.N), torch.uint8)
            met, cnt = _zeros((nb, d.L), torch.float32), _zeros((nb,), torch.int32)
            flags, out8 = _zeros((nb,), torch.uint8), _zeros((8,), torch.int64)
            _sync()
            d.generate_device(par, nb, llr.data_ptr(), info_tx.data_ptr(), cw_tx.data_ptr(), seed=SW_SEED, word0=word,
                              channel=channel)
            d.decode_device(llr.data_ptr(), nb, info.data_ptr(), cw.data_ptr(), met.data_ptr(), cnt.data_ptr())
            d.count_device(info_tx.data_ptr(), cw_tx.data_ptr(), llr.data_ptr(), info.data_ptr(), cw.data_ptr(),
                           cnt.data_ptr(), nb, out8.data_ptr(), flags.data_ptr())
            d.sync()
            errs = np.flatnonzero(flags.cpu().numpy() & 1)
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
        recs.append((par, [int(v) for v in c]))
    return recs, starts


@pytest.mark.gpu
def test_gpu_awgn_channel_sweep_is_the_sweep():
    lib = load().lib()
    d = decoder("a8k4", 2)
    tail = (1.0, 0.5, SW_POINTS, SW_WORDS, SW_ERRORS, SW_SEED, 7)
    old = raw_sweep(lib.bchk_polar_sweep_device, d, *tail)
    assert raw_sweep(lib.bchk_polar_sweep_channel_device, d, CL.AWGN, *tail) == old
    assert d.sweep_device(*tail[:5], seed=SW_SEED, batch=7)[0] == old
    assert all(c[1] == SW_ERRORS for _, c in old)


@pytest.mark.gpu
@pytest.mark.parametrize("channel", ["bsc", "rayleigh"])
def test_gpu_channel_sweep_matches_the_loop_at_every_batch(channel):
    """(8, 4), L = 2, three points, every one cut at its third block error: the records are the
    same at batch 1, 7, 64 and 0 and equal the Python loop; on the BSC the raw bit errors are the
    restatement's flips over exactly the counted words."""
    d = decoder("a8k4", 2)
    frm, step = SW_RANGE[channel]
    runs = {b: d.sweep_device(frm, step, SW_POINTS, SW_WORDS, SW_ERRORS, seed=SW_SEED, batch=b, channel=channel)
            for b in (1, 7, 64, 0)}
    recs = runs[1][0]
    print(channel, "sweep:", recs)
    for b in (7, 64, 0):
        assert runs[b][0] == recs, b
    want, starts = loop_sweep(d, channel, frm, step)
    assert recs == want
    assert [r[0] for r in recs] == [frm + i * step for i in range(SW_POINTS)]
    start = 0
    for (par, c), s0 in zip(recs, starts):
        assert c[1] == SW_ERRORS and c[0] < SW_WORDS and s0 == start  # cut by errors; the index runs on
        if channel == "bsc":
            assert c[6] == int(CL.bsc_flips(CL.word_units(d.N, SW_SEED, start, c[0]), par).sum())
        start += c[0]
    for b, (_, secs, words) in runs.items():
        assert secs > 0 and words >= start


# ---------------------------------------------------------------- 6. genie

@pytest.mark.gpu
@pytest.mark.parametrize("channel", ["rayleigh", "bsc"])
@pytest.mark.parametrize("name", ["short_n7", "G_A3"])
def test_gpu_genie_run_is_generate_plus_genie_device(name, channel):
    import torch
    d = decoder(name)
    W, w0, par = 100, 37, param_of(channel)
    info, llr = _zeros((W, d.K), torch.uint8), _zeros((W, d.N), torch.float32)
    err, soft = _zeros((d.U,), torch.int64), _zeros((d.U,), torch.int64)
    _sync()
    d.generate_device(par, W, llr.data_ptr(), info.data_ptr(), seed=SEED, word0=w0, channel=channel)
    d.genie_device(info.data_ptr(), llr.data_ptr(), W, err.data_ptr(), soft.data_ptr())
    d.sync()
    err, soft = err.cpu().numpy(), soft.cpu().numpy()
    assert err.sum() > 0
    e_sum, s_sum, at = np.zeros(d.U, np.int64), np.zeros(d.U, np.int64), w0
    for n, batch in ((1, 0), (42, 5), (57, 0)):  # the same words, split unevenly in three calls
        e, s, _ = d.genie_run(par, n, seed=SEED, word0=at, batch=batch, channel=channel)
        e_sum, s_sum, at = e_sum + e.view(np.int64), s_sum + s, at + n
    np.testing.assert_array_equal(e_sum, err)
    np.testing.assert_array_equal(s_sum, soft)
    e, s, _ = d.genie_run(par, W, seed=SEED, word0=w0, channel=channel)
    np.testing.assert_array_equal(e.view(np.int64), err)
    np.testing.assert_array_equal(s, soft)
    if channel == "rayleigh":  # another channel, other statistics
        assert (d.genie_run(par, W, seed=SEED, word0=w0)[1] != soft).any()


@pytest.mark.gpu
def test_gpu_design_genie_for_the_bsc():
    """A^5, K = 16 at p = 0.05: K information symbols, the same set on two calls, and the set is
    the documented ranking (errors, then soft sum, then index) of genie_run's counters over the
    lowest-indices-frozen code."""
    F = load()
    layers, K, p, words = ("A",) * 5, 16, 0.05, 500
    spec, err, soft = F.design_genie(layers, K, p, words, seed=4, channel="bsc")
    again = F.design_genie(layers, K, p, words, seed=4, channel="bsc")
    assert again[0] == spec and (again[1] == err).all() and (again[2] == soft).all()
    lines = spec.strip().split("\n")
    assert lines[0] == "32 16 0 5 0 0" and lines[1] == "A A A A A"
    frozen = [int(ln.split()[1]) for ln in lines[2:]]
    assert all(ln.startswith("1 ") for ln in lines[2:]) and len(set(frozen)) == 32 - K
    assert frozen == rank_frozen(err, soft, K)
    base = "\n".join(lines[:2]) + "\n" + "".join(f"1 {f}\n" for f in range(32 - K))
    e, s, _ = F.PolarListDecoder(base, 1).genie_run(p, words, seed=4, channel="bsc")
    np.testing.assert_array_equal(e, err)
    np.testing.assert_array_equal(s, soft)
    assert err.sum() > 0 and (F.design_genie(layers, K, 2.0, words, seed=4)[1] != err).any()  # not the AWGN counters
    d = F.PolarListDecoder(spec, 4)
    assert (d.N, d.K, d.U) == (32, K, 32)


# ---------------------------------------------------------------- 7. refusals that need a context

@pytest.mark.gpu
def test_gpu_dimension_zero_is_refused_on_every_channel():
    import torch
    F = load()
    d = F.PolarListDecoder(arikan_spec(4, 0), 2)
    t = _zeros((64,), torch.float64)
    for channel in CL.CHANNELS:
        par = param_of(channel)
        with pytest.raises(F.BchkError, match="dimension 0"):
            d.generate_device(par, 2, t.data_ptr(), channel=channel)
        with pytest.raises(F.BchkError, match="dimension 0"):
            d.sweep_device(par, 0.0, 1, 10, 1, channel=channel)
        with pytest.raises(F.BchkError, match="dimension 0"):
            d.genie_run(par, 4, channel=channel)
    d8 = decoder("a8k4")
    for channel in ("awgn", "bsc"):
        with pytest.raises(F.BchkError, match="d_h"):
            d8.generate_device(param_of(channel), 2, t.data_ptr(), channel=channel, d_h=t.data_ptr())
    with pytest.raises(F.BchkError, match="p ="):
        d8.generate_device(0.75, 2, t.data_ptr(), channel="bsc")
    d8.generate_device(0.75, 0, None, channel="rayleigh")  # B = 0 is a no-op, whatever the pointers
    _sync()
    assert not t.cpu().numpy().any()
