"""The tiered fixed-point SC-list decoder (csrc/polar_sclist_q8_tiered.hip behind
bchk_polar_create_q8_tiered, PolarListDecoder(llr="q8", state="tiered_q8")): the int8 contract of
include/bchk.h in the tiered state, layers 1..split of every path in a device-memory workspace
with the LLRs as bytes.

Two references. The LDS int8 decoder (csrc/polar_sclist_q8.hip), itself pinned to the restatement
by tests/test_polar_q8.py, for bulk words: counts, information vectors, codewords and metric bits
must be equal at every split. tests/sclist_q8.py, the restatement of the contract, for a few rows
per case and wherever the LDS decoder refuses the code. The layout and the split rule are restated
below from DESIGN 5.15 / 5.19, not read from the library.
"""
import ctypes as C

import numpy as np
import pytest

import sclist_q8
from bchk_pkg import load
from polar_lib import arikan_spec, awgn_llr
from short_codes import short_spec
from test_polar_mixed import kdir  # noqa: F401
from test_polar_q8 import (SWEEP_B, SWEEP_QMAX, SWEEP_SCALE, SWEEP_SEED, assert_same, noisy_rows, pipeline, q8_decoder,
                           restated)
from test_polar_q8_plain import SMALL as PLAIN_SMALL
from test_polar_tiered import AUTO_CHOICE, SMALL

EINVAL = -1
LDS_MAX = 160 * 1024


def tiered_q8(spec, L, split=None, **kw):
    return load().PolarListDecoder(spec, L, llr="q8", state="tiered_q8", split=split, **kw)


def clamped_share(spec, rows, L):
    """(the restatement's lists over the rows, share of its g steps that clamp)"""
    sclist_q8.STATS.update(g=0, clamped=0)
    want = restated(spec, rows, L)
    return want, sclist_q8.STATS["clamped"] / max(sclist_q8.STATS["g"], 1)


# ---------------------------------------------------------------- the layout, restated

def restated_layout(n, L, K, split):
    """(lds_bytes, workspace_bytes, cwsplit) of polar_q8_tiered_layout."""
    U = 1 << n
    off, w = [], 0
    for lam in range(n + 1):  # packed C_0 (U bits), C_lam (U >> (lam-1) bits): whole 32-bit words
        off.append(w)
        w += ((U if lam == 0 else U >> (lam - 1)) + 31) // 32
    cwall = w
    cwsplit = off[split + 1] if split < n else cwall
    Us = U >> split
    pathS = ((Us + 15) & ~15) + 16 if Us > 1 else 0  # bytes
    nC = cwall - cwsplit
    pathC = nC | 1 if nC else 0  # words
    o_C = pathS * L
    o_idx = o_C + 4 * pathC * L
    o_own = o_idx + split * L
    o_act = (o_own + L + 15) & ~15
    lds = (o_act + 4 * L + 4 * L * max((K + 31) // 32, 1) + 15) & ~15
    w_C = (L * (U - Us) + 15) & ~15
    return lds, (w_C + 4 * L * cwsplit + 255) & ~255, cwsplit


def restated_split(n, L, K):
    """The smallest split whose LDS part fits, then further ones while min(8, 160 KiB / lds) grows."""
    def lds(s):
        return restated_layout(n, L, K, s)[0]

    def waves(s):
        return min(8, LDS_MAX // lds(s))

    s = 1
    while s < n and lds(s) > LDS_MAX:
        s += 1
    while s < n and waves(s + 1) > waves(s):
        s += 1
    return s


# ---------------------------------------------------------------- host side (no GPU needed)

def test_q8_tiered_takes_a_code_past_the_q8_lds_limit():
    """(8192, 4096) at L = 32 is refused by llr="q8" with state="lds"; state="tiered_q8" passes every
    spec and limit check, so what is left to fail is the missing device."""
    import torch
    F = load()
    spec = arikan_spec(13, 4096)
    with pytest.raises(F.BchkError, match="LDS"):
        F.PolarListDecoder(spec, 32, llr="q8")
    if torch.cuda.is_available():
        d = tiered_q8(spec, 32)
        assert 1 <= d.split <= 13 and d.state_info()["lds_bytes"] <= LDS_MAX
        d.close()
    else:
        with pytest.raises(F.BchkError, match="device|HIP"):
            tiered_q8(spec, 32)


def test_q8_tiered_refusals(tmp_path):
    F = load()
    (tmp_path / "k2.txt").write_text("2\n1 0\n1 1\n")
    frozen3 = "1 0\n1 1\n1 2\n"
    for spec, kd, name in (("6 3 0 2 0 0\nG A\n" + frozen3, None, "G"),
                           ("4 1 0 2 0 0\n-k2.txt A\n" + frozen3, str(tmp_path), "-k2.txt")):
        with pytest.raises(F.BchkError, match=rf"all-Arikan.*layer 0 is \"{name}\""):
            tiered_q8(spec, 4, kernel_dir=kd)
    for split in (0, 6, -2):
        with pytest.raises(F.BchkError, match="split -?[0-9]+ out of range"):
            tiered_q8(arikan_spec(5, 16), 4, split=split)
    with pytest.raises(F.BchkError, match="layers unsupported|exceeds 16384"):
        tiered_q8(arikan_spec(15, 16384), 2)
    with pytest.raises(F.BchkError, match="list size"):
        tiered_q8(arikan_spec(5, 16), 33)
    with pytest.raises(F.BchkError, match="LDS"):  # 32 paths of 8192 bytes each stay in LDS
        tiered_q8(arikan_spec(14, 8192), 32, split=1)
    with pytest.raises(ValueError, match="q8.*tiered_q8"):
        F.PolarListDecoder(arikan_spec(5, 16), 4, state="tiered", llr="q8")
    with pytest.raises(ValueError, match="llr"):
        F.PolarListDecoder(arikan_spec(5, 16), 4, state="tiered_q8", llr="f32")


# ---------------------------------------------------------------- GPU: every split

@pytest.mark.gpu
@pytest.mark.parametrize("n,K,dyn,punct", SMALL)
@pytest.mark.parametrize("L", [1, 2, 4, 8, 32])
def test_gpu_q8_tiered_every_split(n, K, dyn, punct, L):
    """Every boundary 1..n against the LDS int8 decoder, the first rows against the restatement.
    n >= 6 has sub-word and whole-word butterflies on both sides of the split; splits n-1 and n put
    the 2-LLR and 1-LLR byte layers into the workspace."""
    assert K == 1 << (n - 1)
    spec = arikan_spec(n, K, dyn=dyn, punct=punct, seed=n * 7 + L)
    rows = noisy_rows(spec, 96, 2.0, seed=10 * n + L)
    want = q8_decoder(spec, L).decode(rows)
    few, share = clamped_share(spec, rows[:3], L)
    print(f"U={1 << n} L={L}: {100 * share:.1f} % of the g steps clamp")
    assert share > 0.10
    assert_same(tuple(a[:3] for a in want), few)
    for split in range(1, n + 1):
        d = tiered_q8(spec, L, split)
        assert d.split == split
        got = d.decode(rows)
        d.close()
        assert_same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("n,K", [(2, 2), (3, 4)])
def test_gpu_q8_tiered_layers_narrower_than_a_word(n, K, L):
    spec = arikan_spec(n, K)
    rng = np.random.default_rng(n)
    rows = rng.integers(-128, 128, (40, 1 << n)).astype(np.int8)
    rows[0] = 0
    want = restated(spec, rows, L)
    for split in range(1, n + 1):
        assert_same(tiered_q8(spec, L, split).decode(rows), want)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4, 8])
@pytest.mark.parametrize("n,K,dyn,amp", PLAIN_SMALL)
def test_gpu_q8_tiered_equals_f32_tiered_without_saturation(n, K, dyn, amp, L):
    """Integer LLRs with U max|llr| <= 127: no g step saturates, every value is exact in f32."""
    U = 1 << n
    spec = arikan_spec(n, K, dyn=dyn, seed=n + dyn)
    rng = np.random.default_rng(7 * n + dyn + L)
    rows = rng.integers(-amp, amp + 1, (70, U)).astype(np.int8)
    rows[0] = 0
    rows[1, ::2] = 0
    assert U * int(np.abs(rows).max()) <= 127
    for split in (1, n):
        f32 = load().PolarListDecoder(spec, L, state="tiered", split=split)
        assert_same(tiered_q8(spec, L, split).decode(rows), f32.decode(rows.astype(np.float32)))


@pytest.mark.gpu
def test_gpu_q8_tiered_full_scale_ties_and_zeros():
    """Equal metrics, zero LLRs and every LLR at the bound: only path indices may break ties,
    never array indices."""
    spec = arikan_spec(7, 64, dyn=4, seed=77)
    rng = np.random.default_rng(5)
    rows = np.where(rng.integers(0, 2, (5, 128)) != 0, 127, -127).astype(np.int8)
    rows[1, ::3] = -128  # read as -127
    rows[2] = 0
    rows[3] = noisy_rows(spec, 1, 1.0, seed=78)[0]
    rows[3, ::2] = 0
    rows[4, 1::2] = 0
    want, share = clamped_share(spec, rows, 8)
    assert share > 0.10
    for split in (1, 3, 7):
        assert_same(tiered_q8(spec, 8, split).decode(rows), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n,K", [(3, 3), (4, 5)])
def test_gpu_q8_tiered_full_lists(n, K):
    """L = 2^K keeps every codeword: every unfrozen phase clones, later ones kill too."""
    spec = arikan_spec(n, K)
    rows = noisy_rows(spec, 40, 0.0, seed=n)
    got = tiered_q8(spec, 1 << K, n).decode(rows)
    assert np.all(got[0] == 1 << K)
    assert_same(got, restated(spec, rows, 1 << K))


@pytest.mark.gpu
def test_gpu_q8_tiered_state_reuse_across_codewords(monkeypatch):
    """Three waves decode 1000 codewords each: nothing of a codeword's arrays or indices may
    reach the next."""
    monkeypatch.setenv("BCHK_POLAR_GRID", "3")
    spec = arikan_spec(6, 32, dyn=5, punct=(1, 7), seed=21)
    rows = noisy_rows(spec, 3000, 2.0, seed=22)
    d = tiered_q8(spec, 8, 6)
    assert d.state_info()["grid"] == 3
    lds = load().PolarListDecoder(spec, 8, llr="q8")
    assert_same(d.decode(rows), lds.decode(rows))


@pytest.mark.gpu
def test_gpu_q8_tiered_shortened_punctured_and_dynamic(kdir):
    spec = short_spec("arikan_n7", kdir)  # 3 shortened, 2 punctured, 4 dynamic constraints
    head = spec.split()
    assert (int(head[4]), int(head[5])) == (3, 2)
    rows = noisy_rows(spec, 4, 2.0, seed=33)
    rows[3] = np.where(rows[3] < 0, -127, 127)  # magnitudes that tie with a shortened symbol's 127
    want = restated(spec, rows, 8)
    for split in (1, 7):
        assert_same(tiered_q8(spec, 8, split).decode(rows), want)
    spec = arikan_spec(6, 29, punct=(1, 7, 9))  # N = 61, K = 29: the byte-wise epilogue
    rows = noisy_rows(spec, 3, 2.0, seed=44)
    want = restated(spec, rows, 4)
    for split in (1, 6):
        assert_same(tiered_q8(spec, 4, split).decode(rows), want)


@pytest.mark.gpu
def test_gpu_q8_tiered_where_both_fit():
    spec = arikan_spec(11, 1024)
    rows = noisy_rows(spec, 4, 2.0, seed=77, qmaxes=(63,))
    d = tiered_q8(spec, 32)
    st = d.state_info()
    print("tiered q8 (2048, 1024) L=32:", st)
    assert st["split"] == restated_split(11, 32, 1024)
    assert_same(d.decode(rows), q8_decoder(spec, 32).decode(rows))


def long_words(d, B, seed):
    """test_polar_q8.noiseless and noisy_rows past the C oracle's U <= 4096: the words come from the
    library's host encoder (pinned to the oracle by tests/test_polar_sclist.py)."""
    info = np.random.default_rng(seed).integers(0, 2, (B, d.K)).astype(np.uint8)
    return info, d.encode(info)


def noiseless(d, seed):
    info, sent = long_words(d, 2, seed)
    cnt, gi, gw, gm = d.decode(np.where(sent != 0, -20, 20).astype(np.int8))
    assert (cnt >= 1).all()
    np.testing.assert_array_equal(gi[:, 0], info)
    np.testing.assert_array_equal(gw[:, 0], sent)
    np.testing.assert_array_equal(gm[:, 0].view(np.uint32), np.zeros(2, np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,L,noisy", [(13, 4096, 32, True), (14, 8192, 8, True), (14, 8192, 32, False)])
def test_gpu_q8_tiered_past_the_q8_lds_limit(n, K, L, noisy):
    F = load()
    spec = arikan_spec(n, K)
    with pytest.raises(F.BchkError, match="LDS"):
        F.PolarListDecoder(spec, L, llr="q8")
    d = tiered_q8(spec, L)
    st = d.state_info()
    print(f"tiered q8 ({1 << n}, {K}) L={L}:", st)
    assert st["lds_bytes"] <= LDS_MAX and st["grid"] >= 1
    noiseless(d, n + L)
    if noisy:  # one word as noisy_rows makes them: |LLR| <= 63, the typical one at half of that
        llr = awgn_llr(long_words(d, 1, n + L)[1], 2.0, K / d.N, seed=n + L + 1)
        rows = F.quantize(llr, 63 / 6.0, 63)
        assert_same(d.decode(rows), restated(spec, rows, L))


# ---------------------------------------------------------------- GPU: layout and split

@pytest.mark.gpu
def test_gpu_q8_tiered_layout_and_auto_split():
    """state_info() against the restated layout at the shapes of the f32 tiered table: creation
    only, nothing is decoded."""
    for (n, L, ask), f32 in AUTO_CHOICE.items():
        K = 1 << (n - 1)
        d = tiered_q8(arikan_spec(n, K), L, ask)
        st = d.state_info()
        d.close()
        split = restated_split(n, L, K) if ask is None else ask
        lds, ws, _ = restated_layout(n, L, K, split)
        assert (st["split"], st["lds_bytes"], st["workspace_bytes"]) == (split, lds, ws), (n, L, ask)
        assert lds <= LDS_MAX
    # one anchor by hand, (16384, 8192) at L = 32 and split 7: per layer 32 arrays, 16384 - 128 bytes
    # of S_1..S_7 per chain of arrays, and 512 + 512 + 256 + 128 + 64 + 32 + 16 + 8 packed words of
    # C_0..C_7; the f32 tiered state takes 2 276 352 bytes at the same split
    assert restated_layout(14, 32, 8192, 7)[2] == 1528
    d = tiered_q8(arikan_spec(14, 8192), 32, 7)
    assert d.state_info()["workspace_bytes"] == 32 * 16256 + 4 * 32 * 1528 == 715_776
    assert AUTO_CHOICE[14, 32, None][:1] + AUTO_CHOICE[14, 32, None][2:] == (7, 2_276_352)
    assert d.scratch_bytes()[0] >= d.state_info()["grid"] * 715_776


# ---------------------------------------------------------------- GPU: sweep and refusals

@pytest.mark.gpu
@pytest.mark.parametrize("channel,param", [("awgn", 1.0), ("bsc", 0.08)])
def test_gpu_q8_tiered_sweep_equals_its_own_pipeline(channel, param):
    spec = arikan_spec(8, 128, dyn=6, seed=8)
    d = tiered_q8(spec, 4)
    want, flags = pipeline(d, channel, param, SWEEP_B, SWEEP_SEED)
    recs, secs, words = d.sweep_device(param, 0.5, 1, SWEEP_B, SWEEP_B + 1, seed=SWEEP_SEED, batch=SWEEP_B,
                                       channel=channel, scale=SWEEP_SCALE, qmax=SWEEP_QMAX)
    print(f"tiered q8 sweep {channel}:", recs)
    assert recs == [(param, want)] and words == SWEEP_B and secs > 0
    assert want[0] == SWEEP_B and want[1] == int((flags & 1).sum())
    lds = q8_decoder(spec, 4).sweep_device(param, 0.5, 1, SWEEP_B, SWEEP_B + 1, seed=SWEEP_SEED, batch=SWEEP_B,
                                           channel=channel, scale=SWEEP_SCALE, qmax=SWEEP_QMAX)
    assert lds[0] == recs and lds[2] == words


@pytest.mark.gpu
def test_gpu_q8_tiered_cross_type_refusals():
    import torch
    F = load()
    lib = F.lib()
    d = tiered_q8(arikan_spec(5, 16), 4)
    buf = torch.zeros((4096,), dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    torch.cuda.synchronize()

    def rejected(rc):
        assert rc == EINVAL
        assert "int8" in lib.bchk_last_error().decode()

    rejected(lib.bchk_polar_decode_device(d.handle, p, 2, p, p, p, p, None))
    host = np.zeros(4096, np.uint8).ctypes.data_as(C.c_void_p)
    rejected(lib.bchk_polar_decode_host(d.handle, host, 2, host, host, host, host))
    out = np.zeros(1, F.POLAR_POINT_DTYPE).ctypes.data_as(C.c_void_p)
    rejected(lib.bchk_polar_sweep_channel_device(d.handle, 0, 1.0, 0.5, 1, 64, 10, 1, 0, out, None, None))
    with pytest.raises(TypeError, match="int8"):
        d.decode(np.zeros((1, 32), np.float32))
    with pytest.raises(ValueError, match="scale"):
        d.sweep_device(1.0, 0.5, 1, 64, 10)
