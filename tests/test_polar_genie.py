"""Genie-aided SC on the GPU (csrc/polar_genie.hip behind bchk_polar_genie_device,
bchk_polar_genie_run) and the Monte-Carlo AWGN design on it (bchk_polar_design_genie).

The checker is tests/genie_lib.py, a numpy / float32 restatement of single-path SC with true
feedback. Its CPU tests tie it to PolarOracle (the checker the GPU list decoder is pinned
against): the first unfrozen symbol it decides wrongly is the first information-bit error of
the L = 1 decode, and the metric of a correctly decoded word is its frozen-symbol penalty. The
GPU tests then ask for the restatement's LLRs bit for bit, for the same two properties against
the shipped L = 1 decoder on the same LLRs, and for counters that are exact integer column sums
whatever the batch split. Everything is exact; nothing here is statistical except the final
designed-against-undesigned comparison, whose counts are recorded in DESIGN.md §5.13."""
import ctypes as C
import os

import numpy as np
import pytest

from bchk_pkg import load
from genie_lib import (GenieCode, column_sums, first_wrong_unfrozen, frozen_penalty, rank_frozen)
from polar_lib import PolarOracle, arikan_spec, awgn_llr, pw_order
from test_polar_design import DESIGN_K, DESIGN_L, DESIGN_LAYERS, DESIGN_SEED, DESIGN_SNR, DESIGN_WORDS, lowest_frozen_spec
from test_polar_mixed import KERNELS, _kernel_text, mixed_spec

NEW = ("bchk_polar_genie_device", "bchk_polar_genie_run", "bchk_polar_design_genie")


@pytest.fixture(scope="module")
def kdir(tmp_path_factory):
    """Kernel files as tests/test_polar_mixed.py makes them, the 16 x 16 extended-BCH kernel also
    as test_polar_design writes it; bch64 is the 64 x 64 one (a search layer)."""
    d = tmp_path_factory.mktemp("genie_kernels")
    for name, K in KERNELS.items():
        (d / f"{name}.txt").write_text(_kernel_text(K))
    b = load()
    b.write_kernel_file(os.path.join(d, "e16.txt"), b.kernel_ebch(4))  # as tests/test_polar_design.py
    return str(d)


def shortened_spec():
    """A^5 with symbols 30 and 31 shortened (u_30 = u_31 = 0 makes both zero), N = 30, K = 16."""
    frozen = sorted(set(pw_order(5)[:14]) | {30, 31})
    assert len(frozen) == 16
    return "30 16 0 5 2 0\nA A A A A\n30 31\n" + "".join(f"1 {f}\n" for f in frozen)


# name -> (spec builder, words, BCHK_POLAR_TRELLIS or None)
CASES = {
    "A3": (lambda: arikan_spec(3, 4), 64, None),
    "A7": (lambda: arikan_spec(7, 64), 64, None),                      # crosses a 64-phase flush
    "k3-A5": (lambda: mixed_spec(("k3", "A", "A", "A", "A", "A"), 48), 64, None),  # U = 96, odd inner stride
    "A6-dyn": (lambda: arikan_spec(6, 30, dyn=5), 64, None),
    "A5-punct": (lambda: arikan_spec(5, 16, punct=(3, 17)), 64, None),
    "A5-short": (shortened_spec, 64, None),
    "k4-A": (lambda: mixed_spec(("k4", "A"), 4), 64, None),
    "A-k4": (lambda: mixed_spec(("A", "k4"), 4), 64, None),
    "bch8-A": (lambda: mixed_spec(("bch8", "A"), 8), 64, None),        # enumeration
    "bch16-A": (lambda: mixed_spec(("bch16", "A"), 16), 64, None),     # trellis
    "A-bch16": (lambda: mixed_spec(("A", "bch16"), 16), 64, None),
    "bch32f-A": (lambda: mixed_spec(("bch32f", "A"), 32), 32, None),
    "bch8-A-trellis": (lambda: mixed_spec(("bch8", "A"), 8), 64, "2"),  # eBCH8 forced through the trellis
}
SNR = 2.0


# ---------------------------------------------------------------- host side (no GPU needed)

def test_new_entry_points_are_exported_and_bound():
    F = load()
    lib = F.lib()
    for s in NEW:
        assert s in F.EXPORTS, s
        assert hasattr(lib, s), s
    for m in ("genie_device", "genie_run"):
        assert callable(getattr(F.PolarListDecoder, m, None)), m
    assert callable(getattr(F, "design_genie", None))


CPU_CODES = ["A7", "A6-dyn", "A5-punct", "A5-short", "k3-A5", "bch8-A", "A-bch16"]


@pytest.mark.parametrize("name", CPU_CODES)
def test_helper_agrees_with_the_list1_oracle(name, kdir):
    """The two properties that tie the restatement to PolarOracle.decode(llr, 1)."""
    spec = CASES[name][0]()
    g, o = GenieCode(spec, kdir), PolarOracle(spec, kdir)
    assert (g.N, g.K, g.U) == (o.N, o.K, o.U)
    info = np.random.default_rng(7).integers(0, 2, (24, g.K)).astype(np.uint8)
    cw = o.encode(info)
    llr = awgn_llr(cw, 1.5, g.K / g.N, seed=3)
    right = 0
    for b in range(len(info)):
        u = g.build_u(info[b])
        np.testing.assert_array_equal(o.encode_unshortened(info[b])[g.symtype == 0], cw[b])
        dec = g.sc_llrs(llr[b], u)
        _, inf, _, met = o.decode(llr[b], 1)
        diff = np.flatnonzero(inf[0] != info[b])
        first = first_wrong_unfrozen(g, dec, u)
        assert first == (int(diff[0]) if len(diff) else None), (name, b)
        if first is None:
            right += 1
            assert np.float32(met[0]).view(np.uint32) == frozen_penalty(g, dec, u).view(np.uint32), (name, b)
    assert 0 < right  # the metric property was exercised


def test_statistics_definitions():
    from genie_lib import decisions_wrong, soft_q
    dec = np.array([1.5, -1.5, 0.0, -0.0, 1e9, -1e9, 2.0 ** -17, 3 * 2.0 ** -18, 100000.0], np.float32)
    for ub in (0, 1):
        u = np.full(len(dec), ub, np.uint8)
        sign = -1 if ub else 1
        assert decisions_wrong(dec, u).tolist() == [(v < 0) != bool(ub) for v in dec.tolist()]
        want = [sign * 98304, -sign * 98304, 0, 0, sign * 2 ** 31, -sign * 2 ** 31, 0, sign * 1, sign * 2 ** 31]
        # 2^-17 * 65536 = 0.5 -> 0 and 0.75 -> 1 (nearest even); the clamp at +-32768
        assert soft_q(dec, u).tolist() == want
    assert rank_frozen(np.array([0, 0, 1, 0]), np.array([5, 9, 99, 5]), 2) == [0, 2]  # err, soft, then index


# ---------------------------------------------------------------- GPU helpers

def _zeros(shape, dtype):
    import torch
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()


class Run:
    """Words [word0, word0 + B) of the stream generated on the device and sent through
    genie_device with both dumps; the tensors stay on the device."""

    def __init__(self, d, B, seed=5, word0=0, snr=SNR):
        import torch
        self.d, self.B = d, B
        self.info_tx = _zeros((B, max(d.K, 1)), torch.uint8)
        self.cw_tx = _zeros((B, d.N), torch.uint8)
        self.llr = _zeros((B, d.N), torch.float32)
        self.err = _zeros((d.U,), torch.int64)
        self.soft = _zeros((d.U,), torch.int64)
        self.dec = _zeros((B, d.U), torch.float32)
        self.u = _zeros((B, d.U), torch.uint8)
        _sync()
        d.generate_device(snr, B, self.llr.data_ptr(), self.info_tx.data_ptr(), self.cw_tx.data_ptr(), seed=seed,
                          word0=word0)
        d.genie_device(self.info_tx.data_ptr(), self.llr.data_ptr(), B, self.err.data_ptr(), self.soft.data_ptr(),
                       self.dec.data_ptr(), self.u.data_ptr())
        d.sync()

    def host(self):
        return tuple(t.cpu().numpy() for t in (self.info_tx, self.cw_tx, self.llr, self.err, self.soft, self.dec,
                                               self.u))


_cache = {}


def case(name, kdir):
    """The decoder, the device run and the restatement's reference of one test code (computed
    once, shared by the tests, left unchanged)."""
    if name not in _cache:
        build, B, trellis = CASES[name]
        spec = build()
        old = os.environ.get("BCHK_POLAR_TRELLIS")
        if trellis:
            os.environ["BCHK_POLAR_TRELLIS"] = trellis
        try:
            d = load().PolarListDecoder(spec, 1, kernel_dir=kdir)
        finally:
            if trellis:
                if old is None:
                    del os.environ["BCHK_POLAR_TRELLIS"]
                else:
                    os.environ["BCHK_POLAR_TRELLIS"] = old
        run = Run(d, B)
        g = GenieCode(spec, kdir)
        info, cw, llr, err, soft, dec, u = run.host()
        want_u = np.stack([g.build_u(info[b]) for b in range(B)])
        want_dec = np.stack([g.sc_llrs(llr[b], want_u[b]) for b in range(B)])
        _cache[name] = dict(spec=spec, d=d, g=g, run=run, info=info, cw=cw, llr=llr, err=err, soft=soft, dec=dec,
                            u=u, want_u=want_u, want_dec=want_dec)
    return _cache[name]


# ---------------------------------------------------------------- the kernel

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_decision_llrs_equal_the_restatement_bit_for_bit(name, kdir):
    c = case(name, kdir)
    np.testing.assert_array_equal(c["u"], c["want_u"])
    np.testing.assert_array_equal(c["dec"].view(np.uint32), c["want_dec"].view(np.uint32))
    # d_u is the encoder's input: through the transform (a K = U code over the same layers, host
    # encoder) it gives the transmitted codeword
    g = c["g"]
    layers = c["spec"].split("\n")[1]
    full = load().PolarListDecoder(f"{g.U} {g.U} 0 {g.nl} 0 0\n{layers}\n", 1, kernel_dir=kdir)
    np.testing.assert_array_equal(full.encode(c["u"])[:, g.symtype == 0], c["cw"])
    wrong = (c["dec"] < 0) != (c["u"] != 0)
    print(name, "symbols with errors:", int(wrong.any(axis=0).sum()), "of", g.U, "| decision errors:", int(wrong.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_counters_are_the_column_sums_of_the_dumps(name, kdir):
    c = case(name, kdir)
    err, soft = column_sums(c["dec"], c["u"])
    np.testing.assert_array_equal(c["err"].view(np.uint64), err)
    np.testing.assert_array_equal(c["soft"], soft)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_shipped_list1_decoder_follows_the_genie_llrs(name, kdir):
    """decode_device at L = 1 on the same LLRs: its first information-bit error is the first
    unfrozen symbol the genie LLRs decide wrongly, and a correctly decoded word's metric is the
    frozen-symbol penalty of the genie LLRs -- exactly, every word."""
    import torch
    c = case(name, kdir)
    d, g, run, B = c["d"], c["g"], c["run"], c["run"].B
    info = _zeros((B, 1, max(d.K, 1)), torch.uint8)
    cw = _zeros((B, 1, d.N), torch.uint8)
    met = _zeros((B, 1), torch.float32)
    cnt = _zeros((B,), torch.int32)
    _sync()
    d.decode_device(run.llr.data_ptr(), B, info.data_ptr(), cw.data_ptr(), met.data_ptr(), cnt.data_ptr())
    d.sync()
    info, met, cnt = info.cpu().numpy(), met.cpu().numpy(), cnt.cpu().numpy()
    assert (cnt == 1).all()
    for b in range(B):
        diff = np.flatnonzero(info[b, 0, :d.K] != c["info"][b, :d.K])
        first = first_wrong_unfrozen(g, c["dec"][b], c["u"][b])
        assert first == (int(diff[0]) if len(diff) else None), (name, b)
        if first is None:
            assert met[b, 0].view(np.uint32) == frozen_penalty(g, c["dec"][b], c["u"][b]).view(np.uint32), (name, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A7", "k3-A5", "bch16-A"])
def test_totals_do_not_depend_on_the_split_or_the_dumps(name, kdir):
    import torch
    c = case(name, kdir)
    d, run, B = c["d"], c["run"], c["run"].B
    cuts = [0, 1, B // 2 + 3, B]  # three uneven calls that accumulate, no dumps
    err, soft = _zeros((d.U,), torch.int64), _zeros((d.U,), torch.int64)
    _sync()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        d.genie_device(run.info_tx[lo:].data_ptr(), run.llr[lo:].data_ptr(), hi - lo, err.data_ptr(), soft.data_ptr())
    d.genie_device(run.info_tx.data_ptr(), run.llr.data_ptr(), 0, err.data_ptr(), soft.data_ptr())  # B = 0: a no-op
    d.sync()
    np.testing.assert_array_equal(err.cpu().numpy(), c["err"])
    np.testing.assert_array_equal(soft.cpu().numpy(), c["soft"])
    # one call without dumps, added into non-zero counters
    d.genie_device(run.info_tx.data_ptr(), run.llr.data_ptr(), B, err.data_ptr(), soft.data_ptr())
    d.sync()
    np.testing.assert_array_equal(err.cpu().numpy(), 2 * c["err"])
    np.testing.assert_array_equal(soft.cpu().numpy(), 2 * c["soft"])


@pytest.mark.gpu
def test_any_list_size_and_any_grid_give_the_same_rows(kdir, monkeypatch):
    c = case("k3-A5", kdir)
    monkeypatch.setenv("BCHK_POLAR_GRID", "3")  # three waves stride over the batch
    d8 = load().PolarListDecoder(c["spec"], 8, kernel_dir=kdir)
    info, cw, llr, err, soft, dec, u = Run(d8, c["run"].B).host()
    np.testing.assert_array_equal(dec.view(np.uint32), c["dec"].view(np.uint32))
    np.testing.assert_array_equal(u, c["u"])
    np.testing.assert_array_equal(err, c["err"])
    np.testing.assert_array_equal(soft, c["soft"])


# ---------------------------------------------------------------- genie_run

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A6-dyn", "bch16-A"])
def test_genie_run_is_generate_plus_genie_device(name, kdir):
    c = case(name, kdir)
    d, W, seed, w0 = c["d"], 100, 9, 37
    _, _, _, err, soft, _, _ = Run(d, W, seed=seed, word0=w0).host()
    for batch in (1, 7, 64, 0):
        e, s, secs = d.genie_run(SNR, W, seed=seed, word0=w0, batch=batch)
        np.testing.assert_array_equal(e.view(np.int64), err, err_msg=f"batch {batch}")
        np.testing.assert_array_equal(s, soft, err_msg=f"batch {batch}")
        assert secs > 0
    W1 = 41
    e1, s1, _ = d.genie_run(SNR, W1, seed=seed, word0=w0)
    e2, s2, _ = d.genie_run(SNR, W - W1, seed=seed, word0=w0 + W1)
    np.testing.assert_array_equal((e1 + e2).view(np.int64), err)
    np.testing.assert_array_equal(s1 + s2, soft)


# ---------------------------------------------------------------- design_genie

def frozen_of(spec):
    lines = spec.strip().split("\n")
    fr = [tuple(int(t) for t in ln.split()) for ln in lines[2:]]
    assert all(len(f) == 2 and f[0] == 1 for f in fr)
    return lines[0], lines[1], [f[1] for f in fr]


@pytest.mark.gpu
@pytest.mark.parametrize("layers,K,words", [(("A",) * 6, 32, 2000), (("-bch8.txt", "A", "A"), 12, 500),
                                            (("A",) * 5, 8, 6),           # few words: many symbols tie at err = 0
                                            (("A",) * 4, 1, 300), (("-k4.txt", "A"), 7, 300)],
                         ids=["A6", "bch8-A-A", "ties", "K1", "K=U-1"])
def test_design_genie_applies_the_ranking_rule(layers, K, words, kdir):
    b = load()
    spec, err, soft = b.design_genie(layers, K, 2.0, words, kernel_dir=kdir, seed=4)
    head, line, frozen = frozen_of(spec)
    U = len(err)
    assert head == f"{U} {K} 0 {len(layers)} 0 0" and line == " ".join(layers)
    assert frozen == rank_frozen(err, soft, K) and len(frozen) == U - K
    if words == 6:
        assert int((err == 0).sum()) > K  # the tie-break decided
    # the statistics are genie_run's over the lowest-indices-frozen code
    base = head + "\n" + line + "\n" + "".join(f"1 {f}\n" for f in range(U - K))
    d0 = b.PolarListDecoder(base, 2, kernel_dir=kdir)
    e, s, _ = d0.genie_run(2.0, words, seed=4)
    np.testing.assert_array_equal(e, err)
    np.testing.assert_array_equal(s, soft)
    d = b.PolarListDecoder(spec, 4, kernel_dir=kdir)  # the text loads
    assert (d.N, d.K, d.U) == (U, K, U)


@pytest.mark.gpu
def test_bad_input_is_rejected_without_touching_the_outputs(kdir):
    import torch
    b = load()
    L = b.lib()
    SENT = 0x5A5A5A5A5A5A5A5A

    def design(layers, K, words=64, room=1 << 16):
        buf = C.create_string_buffer(b"untouched", max(room, 16))
        needed = C.c_size_t(12345)
        err = np.full(256, SENT, np.uint64)
        soft = np.full(256, 77, np.int64)
        rc = L.bchk_polar_design_genie(layers.encode(), kdir.encode(), K, 2.0, words, 1, 0, err.ctypes.data_as(C.c_void_p),
                                       soft.ctypes.data_as(C.c_void_p), buf, room, C.byref(needed))
        clean = (err == SENT).all() and (soft == 77).all() and buf.value == b"untouched"
        return rc, needed.value, clean, buf.value.decode()

    rc, needed, clean, text = design("A A A", 4)
    assert rc == 0 and not clean and needed == len(text) + 1 and text.startswith("8 4 0 3 0 0\nA A A\n1 ")
    for args in (("A A A", 0), ("A A A", -1), ("A A A", 9), ("A -missing.txt", 2), ("A B", 2)):
        assert design(*args)[:3] == (-1, 0, True), args
    assert design("A A A", 4, words=0)[:3] == (-1, 0, True)
    assert design("A A A", 4, words=(1 << 31) + 1)[:3] == (-1, 0, True)
    assert design("A A A", 4, room=needed - 1)[:3] == (-1, needed, True)  # short buffer: needed is set
    assert design("A A A", 4, room=needed)[0] == 0
    rc, _, clean, _ = design("-bch64.txt A", 64)  # a 64 x 64 layer is a search layer
    assert (rc, clean) == (-1, True)
    assert "search layer" in L.bchk_last_error().decode()

    d = b.PolarListDecoder(arikan_spec(3, 4), 1)
    for words in (0, (1 << 31) + 1):
        err = np.full(8, SENT, np.uint64)
        soft = np.full(8, 77, np.int64)
        rc = L.bchk_polar_genie_run(d.handle, 2.0, words, 1, 0, 0, err.ctypes.data_as(C.c_void_p),
                                    soft.ctypes.data_as(C.c_void_p), None)
        assert rc == -1 and (err == SENT).all() and (soft == 77).all()
    t = _zeros((8,), torch.int64)
    assert L.bchk_polar_genie_device(d.handle, t.data_ptr(), t.data_ptr(), (1 << 32), t.data_ptr(), t.data_ptr(), None,
                                     None, None) == -1

    d64 = b.PolarListDecoder(mixed_spec(("bch64", "A"), 64), 1, kernel_dir=kdir)
    B = 2
    info, llr = _zeros((B, d64.K), torch.uint8), _zeros((B, d64.N), torch.float32)
    err, soft = _zeros((d64.U,), torch.int64), _zeros((d64.U,), torch.int64)
    _sync()
    with pytest.raises(b.BchkError, match="search layer"):
        d64.genie_device(info.data_ptr(), llr.data_ptr(), B, err.data_ptr(), soft.data_ptr())
    with pytest.raises(b.BchkError, match="search layer"):
        d64.genie_run(2.0, 4)
    _sync()
    assert not err.cpu().numpy().any() and not soft.cpu().numpy().any()


# ---------------------------------------------------------------- designed against undesigned

# 2^18 design words: the smallest count at which two design seeds (23, 29) gave the same frozen set
# on the MI355X (2^12 .. 2^16 did not)
GENIE_DESIGN_WORDS, GENIE_DESIGN_SEED = 1 << 18, 23


@pytest.mark.gpu
def test_genie_designed_code_beats_lowest_indices_frozen(kdir):
    """test_designed_code_beats_lowest_indices_frozen's set-up -- (e16, A, A, A), K = 64, L = 8, 3 dB,
    2^14 evaluation words of seed 11 -- with the frozen set from design_genie at 3 dB over design
    words of another seed. The genie design against the BEC design is printed, not asserted
    (counts: DESIGN.md §5.13)."""
    b = load()
    assert GENIE_DESIGN_SEED != DESIGN_SEED
    genie, _, _ = b.design_genie(DESIGN_LAYERS, DESIGN_K, DESIGN_SNR, GENIE_DESIGN_WORDS, kernel_dir=kdir,
                                 seed=GENIE_DESIGN_SEED)
    bec, _ = b.design_bec(DESIGN_LAYERS, DESIGN_K, 0.5, kernel_dir=kdir)
    errors = {}
    for name, s in (("genie", genie), ("bec", bec), ("lowest", lowest_frozen_spec(DESIGN_LAYERS, DESIGN_K))):
        d = b.PolarListDecoder(s, DESIGN_L, kernel_dir=kdir)
        recs, _, _ = d.sweep_device(DESIGN_SNR, 0.5, 1, DESIGN_WORDS, 10 ** 9, seed=DESIGN_SEED)
        assert recs[0][1][0] == DESIGN_WORDS
        errors[name] = recs[0][1][1]
        d.close()
    print("block errors over", DESIGN_WORDS, "words at", DESIGN_SNR, "dB:", errors, "| design words", GENIE_DESIGN_WORDS)
    assert errors["lowest"] >= 200
    assert errors["genie"] < errors["lowest"]
