"""The fixed-point SC-list decoder on the GPU (csrc/polar_sclist_q8.hip behind bchk_polar_create_q8,
bchk_polar_decode_q8_*, bchk_polar_quantize_device, bchk_polar_sweep_q8_device) against the
contract of include/bchk.h restated in tests/sclist_q8.py: counts, information vectors, codewords
and metrics, exactly. Where no g step can saturate the lists are also those of the f32 decoder,
bit for bit. tests/test_polar_q8_plain.py pins the restatement itself on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

import sclist_q8
from bchk_pkg import load
from polar_lib import PolarOracle, arikan_spec, awgn_llr
from short_codes import short_spec
from test_polar_mixed import kdir, mixed_spec  # noqa: F401
from test_polar_q8_plain import SMALL

EINVAL = -1
_dec = {}


def q8_decoder(spec, L):
    if (spec, L) not in _dec:
        _dec[spec, L] = load().PolarListDecoder(spec, L, llr="q8")
    return _dec[spec, L]


def restated(spec, rows, L):
    """sclist_q8.decode over the rows, in PolarListDecoder.decode's shapes (metrics as exact f32)."""
    head = spec.split()
    N, K = int(head[0]), int(head[1])
    cnt = np.zeros(len(rows), np.int32)
    info = np.zeros((len(rows), L, K), np.uint8)
    cw = np.zeros((len(rows), L, N), np.uint8)
    met = np.zeros((len(rows), L), np.float32)
    for b, q in enumerate(rows):
        c, i, w, m = sclist_q8.decode(spec, q, L)
        assert np.abs(m).max() < 1 << 24
        cnt[b], info[b, :c], cw[b, :c], met[b, :c] = c, i, w, m
    return cnt, info, cw, met


def assert_same(got, want):
    gc, gi, gw, gm = got
    wc, wi, ww, wm = want
    np.testing.assert_array_equal(gc, wc)
    for b in range(len(wc)):
        c = wc[b]
        np.testing.assert_array_equal(gi[b, :c], wi[b, :c], err_msg=f"info, row {b}")
        np.testing.assert_array_equal(gw[b, :c], ww[b, :c], err_msg=f"codeword, row {b}")
        np.testing.assert_array_equal(gm[b, :c].view(np.uint32), wm[b, :c].view(np.uint32), err_msg=f"metrics, row {b}")


def noisy_rows(spec, B, snr, seed, qmaxes=(31, 63, 127)):
    """B words over AWGN, row b quantised with qmaxes[b % 3] and a scale that puts the typical
    |LLR| (about 3 at these rates and Eb/N0) at half of qmax: the tails clamp in the quantiser and
    the sums of the g steps reach 127 within three layers."""
    o = PolarOracle(spec)
    info = np.random.default_rng(seed).integers(0, 2, (B, o.K)).astype(np.uint8)
    llr = awgn_llr(o.encode(info), snr, max(o.K, 1) / o.N, seed=seed + 1)
    F = load()
    return np.stack([F.quantize(llr[b], qmaxes[b % len(qmaxes)] / 6.0, qmaxes[b % len(qmaxes)]) for b in range(B)])


def check(spec, rows, L):
    sclist_q8.STATS.update(g=0, clamped=0)
    want = restated(spec, rows, L)
    share = sclist_q8.STATS["clamped"] / max(sclist_q8.STATS["g"], 1)
    assert_same(q8_decoder(spec, L).decode(rows), want)
    return share


# ---------------------------------------------------------------- no saturation: the f32 lists

@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4, 8])
@pytest.mark.parametrize("n,K,dyn,amp", SMALL)
def test_gpu_q8_equals_f32_decoder_without_saturation(n, K, dyn, amp, L):
    U = 1 << n
    spec = arikan_spec(n, K, dyn=dyn, seed=n + dyn)
    rng = np.random.default_rng(7 * n + dyn + L)
    rows = rng.integers(-amp, amp + 1, (70, U)).astype(np.int8)  # more words than one wave takes
    rows[0] = 0
    rows[1, ::2] = 0
    assert U * int(np.abs(rows).max()) <= 127
    f32 = load().PolarListDecoder(spec, L)
    assert_same(q8_decoder(spec, L).decode(rows), f32.decode(rows.astype(np.float32)))


# ---------------------------------------------------------------- saturating: the restatement

@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4, 8, 32])
@pytest.mark.parametrize("n", [6, 7, 8])
def test_gpu_q8_matches_restatement_with_saturation(n, L):
    spec = arikan_spec(n, 1 << (n - 1))
    share = check(spec, noisy_rows(spec, 3, 2.0, seed=10 * n + L), L)
    print(f"U={1 << n} L={L}: {100 * share:.1f} % of the g steps clamp")
    assert share > 0.10  # "a sizeable share": the inputs are chosen for it, see noisy_rows


@pytest.mark.gpu
def test_gpu_q8_every_llr_at_full_scale():
    spec = arikan_spec(7, 64)
    rng = np.random.default_rng(5)
    rows = np.where(rng.integers(0, 2, (3, 128)) != 0, 127, -127).astype(np.int8)
    rows[2, ::3] = -128  # read as -127
    assert check(spec, rows, 8) > 0.10


@pytest.mark.gpu
def test_gpu_q8_dynamic_freezing():
    spec = arikan_spec(7, 60, dyn=8, seed=3)
    check(spec, noisy_rows(spec, 3, 1.0, seed=21), 8)


@pytest.mark.gpu
def test_gpu_q8_shortened_and_punctured(kdir):
    spec = short_spec("arikan_n7", kdir)  # 3 shortened, 2 punctured, 4 dynamic constraints
    head = spec.split()
    assert (int(head[4]), int(head[5])) == (3, 2)
    rows = noisy_rows(spec, 4, 2.0, seed=33)
    rows[3] = np.where(rows[3] < 0, -127, 127)  # magnitudes that tie with a shortened symbol's 127
    check(spec, rows, 8)


@pytest.mark.gpu
def test_gpu_q8_bytewise_epilogue():
    spec = arikan_spec(6, 29, punct=(1, 7, 9))  # N = 61, K = 29: neither a multiple of 4
    check(spec, noisy_rows(spec, 3, 2.0, seed=44), 4)


@pytest.mark.gpu
@pytest.mark.parametrize("n,K", [(2, 2), (3, 4)])
def test_gpu_q8_layers_narrower_than_a_word(n, K):
    spec = arikan_spec(n, K)
    rng = np.random.default_rng(n)
    rows = rng.integers(-128, 128, (40, 1 << n)).astype(np.int8)
    rows[0] = 0
    check(spec, rows, 4)
    check(spec, rows, 1)


# ---------------------------------------------------------------- beyond the f32 LDS budget

def noiseless(d, spec, seed):
    o = PolarOracle(spec)
    info = np.random.default_rng(seed).integers(0, 2, (2, o.K)).astype(np.uint8)
    sent = o.encode(info)
    cnt, gi, gw, gm = d.decode(np.where(sent != 0, -20, 20).astype(np.int8))
    assert (cnt >= 1).all()
    np.testing.assert_array_equal(gi[:, 0], info)
    np.testing.assert_array_equal(gw[:, 0], sent)
    np.testing.assert_array_equal(gm[:, 0].view(np.uint32), np.zeros(2, np.uint32))


@pytest.mark.gpu
def test_gpu_q8_2048_at_list_32():
    F = load()
    spec = arikan_spec(11, 1024)
    with pytest.raises(F.BchkError, match="LDS"):
        F.PolarListDecoder(spec, 32)
    d = q8_decoder(spec, 32)
    st = d.state_info()
    print("q8 (2048, 1024) L=32:", st)
    assert st["split"] == 0 and st["workspace_bytes"] == 0 and st["grid"] >= 1
    assert 90_000 <= st["lds_bytes"] <= 98_000 <= 160 * 1024  # (2048 + 16) + 4 * 195 + 4 * 33 bytes per path
    noiseless(d, spec, 1)
    check(spec, noisy_rows(spec, 1, 2.0, seed=77, qmaxes=(63,)), 32)


@pytest.mark.gpu
def test_gpu_q8_4096_at_list_16():
    F = load()
    spec = arikan_spec(12, 2048)
    with pytest.raises(F.BchkError, match="LDS"):
        F.PolarListDecoder(spec, 16)
    d = q8_decoder(spec, 16)
    assert d.state_info()["lds_bytes"] <= 160 * 1024
    noiseless(d, spec, 2)


# ---------------------------------------------------------------- the quantiser

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _zeros(shape, dtype):
    import torch
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("scale,qmax", [(1.0, 63), (0.37, 127), (5.0, 1)])
def test_gpu_quantize_device_equals_numpy(scale, qmax):
    import torch
    F = load()
    d = q8_decoder(arikan_spec(5, 16), 4)
    rng = np.random.default_rng(qmax)
    x = (rng.standard_normal(1003) * 40).astype(np.float32)  # 1003: no multiple of 4 or 64
    x[:16] = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 62.5, 63.5, 1e9, -1e9, np.inf, -np.inf, np.nan, -0.0, 0.1, -0.1]
    x[100:120] = (np.arange(20) - 10 + 0.5) / np.float32(scale)  # near ties after scaling
    t_x, t_q = _dev(x), _zeros((1003 + 8,), torch.int8)
    _sync()
    for off in (0, 1):  # whole 16-byte loads, and a pointer that allows none
        t_q.fill_(-99)
        _sync()
        d.quantize_device(t_x[off:].data_ptr(), 1003 - off, t_q[off:].data_ptr(), scale, qmax)
        d.sync()
        got = t_q.cpu().numpy()
        np.testing.assert_array_equal(got[off:1003], F.quantize(x[off:], scale, qmax))
        assert (got[:off] == -99).all() and (got[1003:] == -99).all()  # nothing written past the ends


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_gpu_q8_refusals(kdir):
    import torch
    F = load()
    lib = F.lib()
    with pytest.raises(F.BchkError, match=r"all-Arikan.*layer 0 is \"-bch8.txt\""):
        F.PolarListDecoder(mixed_spec(("bch8", "A"), 8), 4, kernel_dir=kdir, llr="q8")
    with pytest.raises(ValueError, match="q8"):
        F.PolarListDecoder(arikan_spec(5, 16), 4, state="tiered", llr="q8")
    spec = arikan_spec(5, 16)
    dq, df = q8_decoder(spec, 4), F.PolarListDecoder(spec, 4)
    buf = _zeros((4096,), torch.uint8)
    p = buf.data_ptr()
    _sync()

    def rejected(rc, word):
        assert rc == EINVAL
        assert word in lib.bchk_last_error().decode()

    for qmax in (0, 128):
        with pytest.raises(F.BchkError, match="qmax"):
            dq.quantize_device(p, 16, p, 1.0, qmax)
        with pytest.raises(F.BchkError, match="qmax"):
            dq.sweep_device(1.0, 0.5, 1, 64, 10, scale=4.0, qmax=qmax)
    with pytest.raises(F.BchkError, match="scale"):
        dq.quantize_device(p, 16, p, 0.0)
    # cross-type decode calls, device and host entry points
    rejected(lib.bchk_polar_decode_device(dq.handle, p, 2, p, p, p, p, None), "int8")
    rejected(lib.bchk_polar_decode_q8_device(df.handle, p, 2, p, p, p, p, None), "q8")
    host = np.zeros(4096, np.uint8).ctypes.data_as(C.c_void_p)
    rejected(lib.bchk_polar_decode_host(dq.handle, host, 2, host, host, host, host), "int8")
    rejected(lib.bchk_polar_decode_q8_host(df.handle, host, 2, host, host, host, host), "q8")
    out = np.zeros(1, F.POLAR_POINT_DTYPE).ctypes.data_as(C.c_void_p)
    rejected(lib.bchk_polar_sweep_channel_device(dq.handle, 0, 1.0, 0.5, 1, 64, 10, 1, 0, out, None, None), "int8")
    rejected(lib.bchk_polar_sweep_q8_device(df.handle, 0, 1.0, 0.5, 1, 64, 10, 1, 0, out, None, None, 4.0, 63), "q8")
    with pytest.raises(ValueError, match="scale"):
        dq.sweep_device(1.0, 0.5, 1, 64, 10)
    with pytest.raises(ValueError, match="scale"):
        df.sweep_device(1.0, 0.5, 1, 64, 10, scale=4.0)
    with pytest.raises(TypeError, match="int8"):
        dq.decode(np.zeros((1, 32), np.float32))


# ---------------------------------------------------------------- sweep

SWEEP_B, SWEEP_SEED, SWEEP_SCALE, SWEEP_QMAX = 256, 9, 4.0, 63


def pipeline(d, channel, param, B, seed):
    """generate -> quantize -> decode -> count of words [0, B): (counters [8], flags [B])."""
    import torch
    info_tx, cw_tx = _zeros((B, d.K), torch.uint8), _zeros((B, d.N), torch.uint8)
    llr, q = _zeros((B, d.N), torch.float32), _zeros((B, d.N), torch.int8)
    info, cw = _zeros((B, d.L, d.K), torch.uint8), _zeros((B, d.L, d.N), torch.uint8)
    metric, count = _zeros((B, d.L), torch.float32), _zeros((B,), torch.int32)
    out8, flags = _zeros((8,), torch.int64), _zeros((B,), torch.uint8)
    _sync()
    d.generate_device(param, B, llr.data_ptr(), info_tx.data_ptr(), cw_tx.data_ptr(), seed=seed, word0=0,
                      channel=channel)
    d.quantize_device(llr.data_ptr(), B * d.N, q.data_ptr(), SWEEP_SCALE, SWEEP_QMAX)
    d.decode_device(q.data_ptr(), B, info.data_ptr(), cw.data_ptr(), metric.data_ptr(), count.data_ptr())
    d.count_device(info_tx.data_ptr(), cw_tx.data_ptr(), llr.data_ptr(), info.data_ptr(), cw.data_ptr(),
                   count.data_ptr(), B, out8.data_ptr(), flags.data_ptr())
    d.sync()
    return [int(v) for v in out8.cpu().numpy()], flags.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("channel,param", [("awgn", 1.0), ("bsc", 0.08)])
def test_gpu_q8_sweep_equals_its_own_pipeline(channel, param):
    d = q8_decoder(arikan_spec(6, 32, dyn=5, punct=(1, 7), seed=3), 4)
    want, flags = pipeline(d, channel, param, SWEEP_B, SWEEP_SEED)
    recs, secs, words = d.sweep_device(param, 0.5, 1, SWEEP_B, SWEEP_B + 1, seed=SWEEP_SEED, batch=SWEEP_B,
                                       channel=channel, scale=SWEEP_SCALE, qmax=SWEEP_QMAX)
    print(f"q8 sweep {channel}:", recs)
    assert recs == [(param, want)] and words == SWEEP_B and secs > 0
    errors = int((flags & 1).sum())
    assert want[0] == SWEEP_B and want[1] == errors > 3
    # cut by errors: the point ends with the word that carries the third block error
    (_, c), = d.sweep_device(param, 0.5, 1, SWEEP_B, 3, seed=SWEEP_SEED, batch=SWEEP_B, channel=channel,
                             scale=SWEEP_SCALE, qmax=SWEEP_QMAX)[0]
    assert c[1] == 3 and c[0] < SWEEP_B
    assert flags[c[0] - 1] & 1 and int((flags[:c[0]] & 1).sum()) == 3
