"""Dense dynamic freezing on the GPU: the codes of tests/dense_codes.py -- 33 to 64 constraints
live at once, constraints of 65 and 130 terms -- through every kernel that carries the 64-bit
dynamic-freezing mask (PathRegs::dm, csrc/polar_list_device.h) and through the device encoder's
term loop (csrc/polar_enc_device.h). Everything is compared bit for bit with the C oracle, itself
pinned on these codes to the compiled vendored library (tests/golden/polar_ref_dyn_*) and to a
decoder without masks (tests/test_polar_dense_spec.py); and every list entry any decoder returns
here is a codeword: its information vector, encoded from the specification text term by term,
gives the returned codeword.

  default LDS state   polar_sclist.hip (Arikan), polar_mixed.hip (enumeration + trellis; trellis everywhere)
  tiered states       polar_sclist_tiered.hip, polar_mixed_tiered.hip at every split: the lazy
                      copy-on-write tier around clone_regs' 64-bit copy
  budgeted path       polar_mixed.hip's suspend / resume at every suspension point: the save slot's
                      whole dm (tests/test_polar_budget.py's table, rg[3])
  device encoder      encode, bchk_polar_encode_device, generate_device + count_device

Mutations these tests were seen to catch (on a scratch copy): clone_regs copying the
low word of dm only; build_u without its `q += 64` continuation.
"""
import numpy as np
import pytest

import dense_codes
from bchk_pkg import load
from polar_lib import PolarOracle, awgn_llr
from test_polar_budget import TINY, _decode, _decoder
from test_polar_dense_spec import direct_encode
from test_polar_mixed import _same, kdir  # noqa: F401

pytestmark = pytest.mark.gpu

ARIKAN = list(dense_codes.ARIKAN)
MIXED40 = "dyn_A_bch16_bch8_a40"
BUDGET = "dyn_bch8_A_A_A_a34"
B, SNRS = 32, (1.0, 3.0)

_ref = {}


def reference(name, L, kdir, B=B, snrs=SNRS):
    """(spec, [(llr, the oracle's lists)] per SNR), computed once per (code, list size)."""
    key = (name, L, B, snrs)
    if key not in _ref:
        spec = dense_codes.spec(name)
        o = PolarOracle(spec, kdir)
        info = np.random.default_rng(len(name) + L).integers(0, 2, (B, o.K)).astype(np.uint8)
        cw = o.encode(info)
        rows = []
        for snr in snrs:
            llr = awgn_llr(cw, snr, o.K / o.N, seed=int(snr * 10) + L)
            rows.append((llr, o.decode_batch(llr, L)))
        _ref[key] = spec, rows
    return _ref[key]


def check(name, got, want):
    """The oracle's lists bit for bit, and every entry a codeword of the code."""
    _same(got, want)
    cnt, info, cw, _ = got
    keep = np.arange(info.shape[1])[None, :] < cnt[:, None]
    np.testing.assert_array_equal(direct_encode(name, info[keep]), cw[keep], err_msg="a list entry is no codeword")


# ---------------------------------------------------------------- default LDS state

@pytest.mark.parametrize("L", [1, 2, 8, 32])
@pytest.mark.parametrize("name", ARIKAN)
def test_gpu_dense_arikan_matches_oracle(name, L, kdir):
    spec, rows = reference(name, L, kdir)
    d = load().PolarListDecoder(spec, L)
    for llr, want in rows:
        check(name, d.decode(llr), want)
    d.close()


@pytest.mark.parametrize("trellis", [None, "2"], ids=["default", "trellis-everywhere"])
@pytest.mark.parametrize("L", [1, 4, 8])
def test_gpu_dense_mixed_matches_oracle(L, trellis, kdir, monkeypatch):
    if trellis:
        monkeypatch.setenv("BCHK_POLAR_TRELLIS", trellis)
    spec, rows = reference(MIXED40, L, kdir)
    d = load().PolarListDecoder(spec, L, kernel_dir=kdir)
    for llr, want in rows:
        check(MIXED40, d.decode(llr), want)
    d.close()


# ---------------------------------------------------------------- tiered states, every split

@pytest.mark.parametrize("L", [2, 8, 32])
def test_gpu_dense_tiered_every_split(L, kdir):
    name = "dyn_arikan_n8_a64"
    spec, rows = reference(name, L, kdir)
    for split in range(1, 9):
        d = load().PolarListDecoder(spec, L, state="tiered", split=split)
        assert d.split == split
        for llr, want in rows:
            check(name, d.decode(llr), want)
        d.close()


@pytest.mark.parametrize("L", [1, 4, 8])
def test_gpu_dense_tiered_mixed_every_split(L, kdir):
    spec, rows = reference(MIXED40, L, kdir)
    for split in range(1, len(dense_codes.layers(MIXED40)) + 1):
        d = load().PolarListDecoder(spec, L, kernel_dir=kdir, state="tiered_mixed", split=split)
        assert d.split == split
        for llr, want in rows:
            check(MIXED40, d.decode(llr), want)
        d.close()


# ---------------------------------------------------------------- budgeted path
# 34 constraints live at once, so a suspended wave's dm has its high word in use (bits 32, 33);
# every 8 x 8 layer through the search (BCHK_POLAR_ML=2), the budget of one clock tick: a wave
# suspends after every search round ("rounds") or search item ("items"), see test_polar_budget.py.
# Measured on an MI355X: 64 / 232 / 456 launches per call at L = 1 / 4 / 8, in both modes and at
# both SNRs (a search over an 8 x 8 kernel ends within its first round, so a round is an item
# here), under 0.1 s a case at B = 8: B = 16 stays far within a few seconds.
BUDGET_B = 16


@pytest.mark.parametrize("L", [1, 4, 8])
def test_gpu_dense_tiny_budget_matches_oracle(L, kdir, monkeypatch):
    spec, rows = reference(BUDGET, L, kdir, BUDGET_B, (0.0, 2.0))
    one = _decoder(monkeypatch, spec, L, kdir, "0", ml=2)
    tiny = _decoder(monkeypatch, spec, L, kdir, TINY, ml=2)
    try:
        for (llr, want), snr in zip(rows, (0.0, 2.0)):
            a = _decode(monkeypatch, one, llr)
            assert one.last_launches() == 1
            check(BUDGET, a, want)
            for no_mid in (False, True):
                b = _decode(monkeypatch, tiny, llr, no_mid)
                n = tiny.last_launches()
                print(f"\n{BUDGET} L={L} B={BUDGET_B} {snr} dB {'items' if no_mid else 'rounds'}: {n} launches")
                assert n > 1
                check(BUDGET, b, want)
                _same(b, a)
    finally:
        one.close()
        tiny.close()


# ---------------------------------------------------------------- device encoder

@pytest.mark.parametrize("name", ARIKAN + list(dense_codes.MIXED))
def test_gpu_dense_encoders(name, kdir):
    """The host encoder and the encoder kernel (constraints of 65 terms: the term loop's second
    pass holds one lane; of 130: a third pass) against the oracle and the direct XOR of terms."""
    from test_polar_sim import B_ENC, encode_device
    spec = dense_codes.spec(name)
    o, d = PolarOracle(spec, kdir), load().PolarListDecoder(spec, 1, kernel_dir=kdir)
    info = np.random.default_rng(len(name)).integers(0, 2, (B_ENC, o.K)).astype(np.uint8)
    want = direct_encode(name, info)
    np.testing.assert_array_equal(o.encode(info), want)
    np.testing.assert_array_equal(d.encode(info), want)
    np.testing.assert_array_equal(encode_device(d, info), want)
    d.close()


def test_gpu_dense_generate_and_count():
    """generate_device, decode, count_device once on the (256, 64) code: the generated codewords are
    the information words' (term by term), the eight counters those recomputed on the host."""
    import torch
    from test_polar_sim import Batch, _sync, _zeros, np_counters
    name, n = "dyn_arikan_n8_a64", 256
    d = load().PolarListDecoder(dense_codes.spec(name), 4)
    # 2 dB: the C oracle at L = 4 loses 97 of 256 words there (numpy's AWGN), so both kinds of word occur
    bt = Batch(d, 2.0, n, seed=11)
    out8, flags = _zeros((8,), torch.int64), _zeros((n,), torch.uint8)
    _sync()
    bt.count_device(0, n, out8, flags)
    host = bt.host()
    np.testing.assert_array_equal(direct_encode(name, host[0]), host[1])
    per, want_flags = np_counters(*host)
    got = out8.cpu().numpy()
    print("dense counters:", got.tolist())
    np.testing.assert_array_equal(got, per.sum(axis=0))
    np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)
    assert got[0] == n and 0 < got[1] < n
    d.close()
