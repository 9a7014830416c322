"""Polar FER simulation on the GPU (csrc/polar_channel.hip behind bchk_polar_encode_device,
bchk_polar_generate_device, bchk_polar_count_device, bchk_polar_sweep_device): the encoder
against the C restatement and the host encoder bit for bit, the counter-based word stream
(range splitting, noise statistics, the stored rounding), the simulator's eight counters
against a numpy restatement of include/bchk.h's table computed from the same device outputs,
and the sweep against a word-by-word loop over generate / decode / those counters.

The statistical bounds are 5 standard errors of the sample sizes used (stated where they are
formed); everything else is exact.
"""
import ctypes as C

import numpy as np
import pytest

from bchk_pkg import load
from polar_lib import PolarOracle, arikan_spec
from test_polar_mixed import KERNELS, kdir, mixed_spec  # noqa: F401
from test_polar_sclist import CODES as ARIKAN_CODES

NEW = ("bchk_polar_encode_device", "bchk_polar_generate_device", "bchk_polar_count_device",
       "bchk_polar_sweep_device")
SIM_CODE = (6, 32, 5, (1, 7))  # n, K, dynamic constraints, punctured: N = 62
SNR, L_SIM = 1.0, 4


# ---------------------------------------------------------------- host side (no GPU needed)

def test_new_entry_points_are_exported_and_bound():
    F = load()
    lib = F.lib()  # (imports torch first: one HIP runtime for the whole process)
    for s in NEW:
        assert s in F.EXPORTS, s
        assert hasattr(lib, s), s
    for m in ("encode_device", "generate_device", "count_device", "sweep_device"):
        assert callable(getattr(F.PolarListDecoder, m, None)), m


# ---------------------------------------------------------------- GPU helpers

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _zeros(shape, dtype):
    import torch
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()


def encode_device(d, info):
    import torch
    t_info = _dev(info) if d.K else _zeros((max(len(info), 1),), torch.uint8)
    t_cw = _zeros((len(info), d.N), torch.uint8)
    _sync()
    d.encode_device(t_info.data_ptr(), len(info), t_cw.data_ptr())
    d.sync()
    return t_cw.cpu().numpy()


def generate(d, snr, B, seed=1, word0=0, want_info=True, want_cw=True):
    """(info [B][K], cw [B][N], llr [B][N]) of words [word0, word0 + B), as numpy arrays."""
    import torch
    t_info = _zeros((B, d.K), torch.uint8) if want_info else None
    t_cw = _zeros((B, d.N), torch.uint8) if want_cw else None
    t_llr = _zeros((B, d.N), torch.float32)
    _sync()
    d.generate_device(snr, B, t_llr.data_ptr(), t_info.data_ptr() if want_info else None,
                      t_cw.data_ptr() if want_cw else None, seed=seed, word0=word0)
    d.sync()
    return (t_info.cpu().numpy() if want_info else None, t_cw.cpu().numpy() if want_cw else None,
            t_llr.cpu().numpy())


class Batch:
    """Words [word0, word0 + B) generated and decoded on the device; the tensors stay there."""

    def __init__(self, d, snr, B, seed, word0=0):
        import torch
        self.d, self.B = d, B
        self.info_tx = _zeros((B, d.K), torch.uint8)
        self.cw_tx = _zeros((B, d.N), torch.uint8)
        self.llr = _zeros((B, d.N), torch.float32)
        self.info = _zeros((B, d.L, d.K), torch.uint8)
        self.cw = _zeros((B, d.L, d.N), torch.uint8)
        self.metric = _zeros((B, d.L), torch.float32)
        self.count = _zeros((B,), torch.int32)
        _sync()
        d.generate_device(snr, B, self.llr.data_ptr(), self.info_tx.data_ptr(), self.cw_tx.data_ptr(), seed=seed,
                          word0=word0)
        d.decode_device(self.llr.data_ptr(), B, self.info.data_ptr(), self.cw.data_ptr(), self.metric.data_ptr(),
                        self.count.data_ptr())
        d.sync()

    def count_device(self, lo, hi, out8, flags=None):
        """Counters of words [lo, hi) of the batch added into the device tensor out8."""
        d, n = self.d, hi - lo
        self.d.count_device(self.info_tx[lo:].data_ptr(), self.cw_tx[lo:].data_ptr(), self.llr[lo:].data_ptr(),
                            self.info[lo:].data_ptr(), self.cw[lo:].data_ptr(), self.count[lo:].data_ptr(), n,
                            out8.data_ptr(), flags[lo:].data_ptr() if flags is not None else None)
        d.sync()

    def host(self):
        return tuple(t.cpu().numpy() for t in (self.info_tx, self.cw_tx, self.llr, self.info, self.cw, self.count))


def np_counters(info_tx, cw_tx, llr, info, cw, count):
    """include/bchk.h's table of bchk_polar_count_device, word by word: (per-word contributions
    [B][8], flags [B])."""
    B, N = cw_tx.shape
    per = np.zeros((B, 8), np.int64)
    flags = np.zeros(B, np.uint8)
    for b in range(B):
        per[b, 0] = 1
        z = np.where(cw_tx[b] != 0, -llr[b], llr[b])
        per[b, 6] = int((z < 0).sum())
        if count[b] <= 0:
            per[b, 1] = per[b, 5] = per[b, 7] = 1
            flags[b] = 1 | 4
            continue
        ibe = int(((info[b, 0] != 0) != (info_tx[b] != 0)).sum())
        if not ibe:
            continue
        per[b, 1], per[b, 2] = 1, ibe
        per[b, 3] = int(((cw[b, 0] != 0) != (cw_tx[b] != 0)).sum())
        f = 1
        ml = cur = 0.0  # double sums in index order
        for i in range(N):
            v = float(llr[b, i])
            ml += -v if cw_tx[b, i] else v
            cur += -v if cw[b, 0, i] else v
        if cur >= ml:
            per[b, 4] = 1
            f |= 2
        if not any(np.array_equal(cw[b, r] != 0, cw_tx[b] != 0) for r in range(1, int(count[b]))):
            per[b, 5] = 1
            f |= 4
        flags[b] = f
    return per, flags


_ctx = {}


def sim_decoder():
    if "d" not in _ctx:
        n, K, dyn, punct = SIM_CODE
        spec = arikan_spec(n, K, dyn=dyn, punct=punct, seed=3)
        _ctx["d"] = (spec, load().PolarListDecoder(spec, L_SIM))
    return _ctx["d"]


# ---------------------------------------------------------------- 1. encoder

MIXED = [
    (("k4", "A"), 4, 0, ()),
    (("A", "k8", "A"), 14, 3, (5, 9)),   # punctured
    (("k3", "k4", "A"), 12, 2, ()),      # odd kernel size, U = 24: no whole 32-bit word
    (("bch16", "bch8"), 64, 4, ()),
    (("A", "bch32f"), 30, 2, (7,)),      # an Arikan layer of stride 32 over a matrix layer
    (("bch64f", "A"), 60, 2, (5, 77)),   # the 64 x 64 kernel: encode only
    (("A", "bch64f"), 64, 2, ()),
    (("A", "k3"), 3, 1, ()),             # an Arikan layer whose stride is no power of two
]
B_ENC = 70  # 4 waves per workgroup: the last workgroup is partial


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,dyn,punct", ARIKAN_CODES)
def test_gpu_encoder_arikan(n, K, dyn, punct):
    spec = arikan_spec(n, K, dyn=dyn, punct=punct, seed=n)
    o, d = PolarOracle(spec), load().PolarListDecoder(spec, 1)
    info = np.random.default_rng(n).integers(0, 2, (B_ENC, K)).astype(np.uint8)
    got = encode_device(d, info)
    np.testing.assert_array_equal(got, o.encode(info))
    np.testing.assert_array_equal(got, d.encode(info))


@pytest.mark.gpu
@pytest.mark.parametrize("layers,K,dyn,punct", MIXED, ids=["-".join(c[0]) for c in MIXED])
def test_gpu_encoder_mixed(kdir, layers, K, dyn, punct):
    spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 11 + K)
    o, d = PolarOracle(spec, kdir), load().PolarListDecoder(spec, 1, kernel_dir=kdir)
    info = np.random.default_rng(K).integers(0, 2, (B_ENC, K)).astype(np.uint8)
    got = encode_device(d, info)
    np.testing.assert_array_equal(got, o.encode(info))
    np.testing.assert_array_equal(got, d.encode(info))


@pytest.mark.gpu
def test_gpu_encoder_length_16384():
    """U = 16384 (the oracle stops at 4096): against the host encoder; L = 1 fits the LDS."""
    spec = arikan_spec(14, 8192, dyn=40, punct=(3, 9000), seed=14)
    d = load().PolarListDecoder(spec, 1)
    assert (d.U, d.N, d.K) == (16384, 16382, 8192)
    info = np.random.default_rng(14).integers(0, 2, (B_ENC, 8192)).astype(np.uint8)
    np.testing.assert_array_equal(encode_device(d, info), d.encode(info))


# ---------------------------------------------------------------- 2. the word stream

def _stream_checks(spec, B, cut):
    o, d = PolarOracle(spec), load().PolarListDecoder(spec, 1)
    info, cw, llr = generate(d, SNR, B, seed=7)
    np.testing.assert_array_equal(cw, o.encode(info))
    a, b = generate(d, SNR, cut, seed=7), generate(d, SNR, B - cut, seed=7, word0=cut)
    for whole, p0, p1 in zip((info, cw, llr.view(np.uint32)), a, b):
        np.testing.assert_array_equal(whole, np.concatenate([p0.view(whole.dtype), p1.view(whole.dtype)]))
    # d_info and d_cw are optional: the LLRs do not depend on them
    np.testing.assert_array_equal(generate(d, SNR, 100, seed=7, want_info=False, want_cw=False)[2].view(np.uint32),
                                  llr[:100].view(np.uint32))
    return d, info, cw, llr


@pytest.mark.gpu
def test_gpu_stream_even_length():
    n, K, dyn, punct = SIM_CODE
    B = 4096
    d, info, cw, llr = _stream_checks(arikan_spec(n, K, dyn=dyn, punct=punct, seed=3), B, 1237)
    assert d.N == 62
    i2, c2, l2 = generate(d, SNR, 256, seed=8)
    assert (i2 != info[:256]).any() and (l2 != llr[:256]).any()  # two seeds differ
    # noise recovered from the LLRs: z = (-llr var / 2 - x) / sigma
    sigma = np.sqrt(0.5 * 10.0 ** (-SNR / 10.0) * d.N / d.K)
    var = sigma * sigma
    x = np.where(cw != 0, 1.0, -1.0)
    y = -llr.astype(np.float64) * var / 2.0
    z = (y - x) / sigma
    cnt = z.size  # 4096 * 62 samples: standard errors 1 / sqrt(cnt) (mean), sqrt(2 / cnt) (variance)
    assert abs(z.mean()) < 5.0 / np.sqrt(cnt)
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / cnt)
    assert abs((z * x).mean()) < 5.0 / np.sqrt(cnt)  # x = +-1: z x is standard normal too
    assert abs(info.mean() - 0.5) < 5.0 * 0.5 / np.sqrt(info.size)
    assert abs(cw.mean() - 0.5) < 0.05  # BPSK carries both signs
    # the stored value is float32(-2 y / var) of the double y
    np.testing.assert_array_equal((-2.0 * y / var).astype(np.float32).view(np.uint32), llr.view(np.uint32))


@pytest.mark.gpu
def test_gpu_stream_odd_length():
    """N = 63: the Box-Muller pairs straddle the words and the split (1237 * 63 is odd)."""
    d, info, cw, llr = _stream_checks(arikan_spec(6, 32, dyn=5, punct=(1,), seed=3), 2048, 1237)
    assert d.N == 63


# ---------------------------------------------------------------- 3. counters

SEED_CNT = 1


@pytest.mark.gpu
def test_gpu_counters_match_numpy():
    """(62, 32) L = 4 at 1.0 dB, 512 words of stream SEED_CNT. On the MI355X this seed gave
    (words, block, info bit, code bit, ML, list, raw, no decision) =
    (512, 141, 1449, 1402, 137, 62, 4116, 0): 4 block errors are not ML errors and 79 have the
    sent codeword further down the list, so no condition below holds vacuously."""
    import torch
    spec, d = sim_decoder()
    B = 512
    bt = Batch(d, SNR, B, SEED_CNT)
    out8 = _zeros((8,), torch.int64)
    flags = _zeros((B,), torch.uint8)
    _sync()
    bt.count_device(0, B, out8, flags)
    got = out8.cpu().numpy()
    per, want_flags = np_counters(*bt.host())
    print("polar counters:", got.tolist())
    np.testing.assert_array_equal(got, per.sum(axis=0))
    np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)
    words, blk, ibe, cbe, ml, lst, raw, nodec = (int(v) for v in got)
    assert words == B
    assert 0 < ml < blk and 0 < lst < blk and raw > 0 and cbe > 0 and ibe > 0, got.tolist()
    # two halves into one accumulator; d_flags = NULL
    half = _zeros((8,), torch.int64)
    _sync()
    bt.count_device(0, 200, half)
    bt.count_device(200, B, half)
    np.testing.assert_array_equal(half.cpu().numpy(), got)


@pytest.mark.gpu
def test_gpu_counters_words_without_decision():
    """count <= 0 adds to words, block errors, list errors, raw bit errors and [7] only."""
    import torch
    spec, d = sim_decoder()
    B = 64
    bt = Batch(d, SNR, B, SEED_CNT)
    bt.count[::3] = 0
    bt.count[1::7] = -1
    out8, flags = _zeros((8,), torch.int64), _zeros((B,), torch.uint8)
    _sync()
    bt.count_device(0, B, out8, flags)
    per, want_flags = np_counters(*bt.host())
    assert per[:, 7].sum() > 20
    np.testing.assert_array_equal(out8.cpu().numpy(), per.sum(axis=0))
    np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)


# ---------------------------------------------------------------- 4. sweep

POINTS, MAX_WORDS, MAX_ERRORS, SEED_SWEEP = 3, 3000, 40, 5


def _reference_sweep(d, snr_from, snr_step, points, max_words, max_errors, seed):
    """Word by word: generate, decode, count; a point ends with the word carrying the
    max_errors-th block error (or after max_words), the next starts at the following word."""
    recs, word, last = [], 0, []
    for pt in range(points):
        snr = snr_from + pt * snr_step
        c = np.zeros(8, np.int64)
        while c[0] < max_words and c[1] < max_errors:
            nb = int(min(500, max_words - c[0]))
            per, flags = np_counters(*Batch(d, snr, nb, seed, word0=word).host())
            used = nb
            for w in range(nb):  # walk the words in order
                c += per[w]
                if c[1] >= max_errors:
                    used = w + 1
                    break
            word += used
            last_flag = int(flags[used - 1])
        recs.append((snr, [int(v) for v in c]))
        last.append((word, last_flag))
    return recs, last


@pytest.mark.gpu
def test_gpu_sweep_matches_word_by_word_loop():
    spec, d = sim_decoder()
    runs = {b: d.sweep_device(SNR, 0.5, POINTS, MAX_WORDS, MAX_ERRORS, seed=SEED_SWEEP, batch=b)
            for b in (64, 37, 3000)}
    recs = runs[64][0]
    for b in (37, 3000):
        assert runs[b][0] == recs, b
    want, last = _reference_sweep(d, SNR, 0.5, POINTS, MAX_WORDS, MAX_ERRORS, SEED_SWEEP)
    print("polar sweep:", recs)
    assert recs == want
    start = 0
    for (snr, c), (end, last_flag) in zip(recs, last):
        assert c[0] == end - start  # each point starts at the word after the previous point's last
        start = end
        if c[1] >= MAX_ERRORS:  # cut by errors: exactly there, and the last word is an errored one
            assert c[1] == MAX_ERRORS and c[0] <= MAX_WORDS and (last_flag & 1)
        else:                   # cut by words
            assert c[0] == MAX_WORDS
    assert [r[0] for r in recs] == [1.0, 1.5, 2.0]
    assert any(c[1] == MAX_ERRORS for _, c in recs)
    for b, (_, secs, words) in runs.items():
        assert secs > 0 and words >= sum(c[0] for _, c in recs)


@pytest.mark.gpu
def test_gpu_sweep_point_cut_by_words():
    spec, d = sim_decoder()
    recs, _, words = d.sweep_device(SNR, 0.5, 2, 300, 10 ** 6, seed=SEED_SWEEP, batch=128)
    want, _ = _reference_sweep(d, SNR, 0.5, 2, 300, 10 ** 6, SEED_SWEEP)
    assert recs == want and [c[0] for _, c in recs] == [300, 300] and words == 600
    assert all(0 < c[1] < 300 for _, c in recs)


# ---------------------------------------------------------------- 5. bad arguments

@pytest.mark.gpu
def test_gpu_bad_arguments():
    import torch
    F = load()
    lib = F.lib()
    spec, d = sim_decoder()
    buf = _zeros((4 * 64 * 8,), torch.uint8)
    p = buf.data_ptr()
    EINVAL = -1

    def rejected(rc):
        assert rc == EINVAL
        assert lib.bchk_last_error().decode()

    rejected(lib.bchk_polar_encode_device(d.handle, None, 4, p, None))
    rejected(lib.bchk_polar_encode_device(d.handle, p, 4, None, None))
    rejected(lib.bchk_polar_encode_device(None, p, 4, p, None))
    rejected(lib.bchk_polar_generate_device(d.handle, 1.0, 4, 1, 0, None, None, None, None))
    rejected(lib.bchk_polar_generate_device(d.handle, 1.0, 1 << 32, 1, 0, None, None, p, None))
    for missing in range(7):  # every required pointer of count_device in turn (d_flags may be NULL)
        args = [p] * 7
        args[missing] = None
        rejected(lib.bchk_polar_count_device(d.handle, *args[:6], 4, args[6], None, None))
    rejected(lib.bchk_polar_sweep_device(d.handle, 1.0, 0.5, 0, 100, 10, 1, 0, None, None, None))
    out = np.zeros(1, F.POLAR_POINT_DTYPE)
    rejected(lib.bchk_polar_sweep_device(d.handle, 1.0, 0.5, 1, 100, 10, 1, 0, None, None, None))
    rejected(lib.bchk_polar_sweep_device(d.handle, 1.0, 0.5, 0, 100, 10, 1, 0, out.ctypes.data_as(C.c_void_p),
                                         None, None))
    # B = 0 is a no-op, whatever the pointers
    assert lib.bchk_polar_encode_device(d.handle, None, 0, None, None) == 0
    assert lib.bchk_polar_generate_device(d.handle, 1.0, 0, 1, 0, None, None, None, None) == 0
    assert lib.bchk_polar_count_device(d.handle, None, None, None, None, None, None, 0, None, None, None) == 0
