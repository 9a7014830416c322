"""Polar codes over the library's named kernels G (3 x 3) and A5 (5 x 5)
(out/external/Kernel.cpp:234-274, TruncatedArikanKernel.cpp), pinned to the reference itself by
tests/golden/named_ref_*.txt.gz (tests/named_lib.py; written by scripts/make_named_golden.py).

  CPU   the fixtures regenerate byte for byte where oracle/_ref/polar_ref exists; the kernel
        rows the product uses reproduce every '@encode' section (which settles A5's rows: the
        reference's A5[] array disagrees with what it encodes with); names parse in any case;
        the BEC design refuses a named kernel by name.
  GPU   PolarListDecoder over G / A5 specifications against every fixture at every recorded list
        size: count, information vectors, codewords, list order, f32 metric bits; both encoders;
        G in an outer layer with a list against the matrix form of the same code; budgeted
        launches; the genie kernel against the L = 1 decoder; the simulation loop; design_genie.
"""
import ctypes as C
import os

import numpy as np
import pytest

import named_lib as NL
import polar_ref_lib as R
from bchk_pkg import load
from test_polar_reference import assert_lists_equal

NAMED, OUTER = NL.named_files(), NL.outer_files()
CASES = [(p, L) for p in NAMED for L in NL.fixture(p).list_sizes]
_case_ids = [f"{NL.ident(p)}-L{L}" for p, L in CASES]
OUTER_CASES = [(p, L) for p in OUTER for L in NL.fixture(p).list_sizes]
_outer_ids = [f"{NL.ident(p)}-L{L}" for p, L in OUTER_CASES]
BCHK_EINVAL, BCHK_ENODEV = -1, -2


@pytest.fixture(scope="module")
def kdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("named_kernels")
    for p in NAMED + OUTER:
        NL.fixture(p).write_kernels(str(d))
    return str(d)


def fx_named(name):
    return NL.fixture(os.path.join(R.GOLD, f"named_ref_{name}.txt.gz"))


# ------------------------------------------------------------------ CPU

def test_the_fixture_set_is_the_one_the_generator_writes():
    assert sorted(NL.ident(p) for p in NAMED) == sorted(c[0] for c in NL.CASES)
    assert sorted(NL.ident(p) for p in OUTER) == sorted(c[0] for c in NL.OUTER_CASES)
    for name, layers, K, lists, _ in NL.CASES:
        fx = fx_named(name)
        assert fx.list_sizes == list(lists) and len(fx.llr) == NL.ROWS and len(fx.info) == NL.ENC_WORDS
        assert fx.spec.split("\n")[1].split() == list(layers) and int(fx.spec.split()[1]) == K
        # no list is recorded where the reference's G state does not survive a clone: G is the
        # innermost layer, or the list size is 1
        assert "G" not in layers[:-1] or list(lists) == [1], name
    for name, layers, K, lists in NL.OUTER_CASES:
        fx = fx_named(name)
        assert fx.list_sizes == list(lists) and fx.spec.split("\n")[1].split() == list(layers)
        assert (1.0 - NL.OUTER_MAX_DROP) * NL.OUTER_ROWS <= len(fx.llr) <= NL.OUTER_ROWS
        for L in lists:
            assert all(NL.list_metric_gap(m) >= NL.OUTER_GAP for _, _, _, m in fx.decoded(L))


def test_fixtures_exercise_what_they_are_for():
    for p in NAMED:
        fx = NL.fixture(p)
        L = max(fx.list_sizes)
        rows = fx.decoded(L)
        assert all(c >= 1 for c, *_ in rows)
        if L > 1:
            assert max(c for c, *_ in rows) > 1
    for name in ("A_A5_A_ties", "A_A_G_ties"):
        t = fx_named(name)
        assert np.all(t.llr % 4 == 0) and np.any(t.llr == 0)
        assert any(len(set(m.tolist())) < len(m) for _, _, _, m in t.decoded(8))
    s = fx_named("A_G_A5_A").spec.split("\n")
    assert s[0] == "57 30 0 4 1 2" and s[2] == "59 0 7" and fx_named("A_G_A5_A").spec.count("\n3 ") == 2


@pytest.mark.parametrize("path", NAMED + OUTER, ids=NL.ident)
def test_fixture_regenerates_byte_for_byte(path, tmp_path):
    why = R.ref_lacks("decode")
    if why:
        pytest.skip(why)
    fx = NL.fixture(path)
    again = R.regenerate(fx, str(tmp_path))
    assert again.dumps() == fx.dumps()
    out = tmp_path / "again.txt.gz"
    again.save(str(out))
    assert out.read_bytes() == open(path, "rb").read()


def _transform(spec, kernels, u, a5=NL.A5):
    """CMixedKernelEncoder::Encode's transform (MixedKernelEncoder.cpp:159-170), innermost layer
    first: each block of stride * l symbols, as l rows of `stride`, becomes rows x kernel."""
    mats = {"A": np.array([[1, 0], [1, 1]], np.uint8), "G": NL.G, "A5": a5}
    names = spec.split("\n")[1].split()
    stride = 1
    for n in reversed(names):
        Km = mats[n] if n in mats else kernels[n[1:]]
        l = len(Km)
        blocks = u.reshape(-1, l, stride)
        u = (np.einsum("bjs,ji->bis", blocks.astype(np.int64), Km.astype(np.int64)) & 1).astype(np.uint8).reshape(-1)
        stride *= l
    return u


@pytest.mark.parametrize("path", NAMED, ids=NL.ident)
def test_kernel_rows_reproduce_the_reference_encoder(path):
    """The rows of csrc/polar_host.cpp read_kernel (restated in named_lib) against '@encode':
    for A5 the matrix CA5Kernel::Multiply implements, not the A5[] array GetKernel() returns."""
    fx = NL.fixture(path)
    tok = fx.spec.split()
    N, K, _, nl, nsh, npu = (int(t) for t in tok[:6])
    U = N + nsh + npu
    pos = 6 + nl
    dropped = [int(t) for t in tok[pos:pos + nsh + npu]]
    pos += nsh + npu
    cons = {}
    for _ in range(U - K):
        w = int(tok[pos])
        terms = [int(t) for t in tok[pos + 1:pos + 1 + w]]
        cons[terms[-1]] = terms[:-1]
        pos += 1 + w
    keep = [i for i in range(U) if i not in dropped]
    as_array = []  # the words as the A5[] array's rows (3 and 4 exchanged) would encode them
    for info, want in zip(fx.info, fx.encoded):
        u, k = np.zeros(U, np.uint8), 0
        for i in range(U):
            if i in cons:
                for t in cons[i]:
                    u[i] ^= u[t]
            else:
                u[i] = info[k]
                k += 1
        np.testing.assert_array_equal(_transform(fx.spec, fx.kernels, u)[keep], want)
        as_array.append(np.array_equal(_transform(fx.spec, fx.kernels, u, NL.A5[[0, 1, 2, 4, 3]])[keep], want))
    if "A5" in tok[6:6 + nl]:
        assert not all(as_array)


def _create(spec, L=1):
    lib = load().lib()
    h = C.c_void_p()
    rc = lib.bchk_polar_create_kdir(spec.encode(), None, L, 0, C.byref(h))
    msg = lib.bchk_last_error().decode() if rc else ""
    if rc == 0:
        lib.bchk_polar_destroy(h)
    return rc, msg


@pytest.mark.parametrize("names,U", [("G", 3), ("g", 3), ("A5", 5), ("a5", 5), ("g a5 A", 30), ("a G A5", 30)])
def test_names_parse_in_any_case(names, U):
    """The specification is checked before the device is looked for: with no GPU a good one
    ends in BCHK_ENODEV, never in 'Unknown kernel'."""
    spec = f"{U} {U - 1} 0 {len(names.split())} 0 0\n{names}\n1 0\n"
    rc, msg = _create(spec)
    assert rc in (0, BCHK_ENODEV) and "Unknown kernel" not in msg, msg
    rc, msg = _create(spec.replace(f"{U} {U - 1}", f"{U + 1} {U - 1}"))
    assert rc == BCHK_EINVAL and "Code length mismatch" in msg  # the size each name stands for


@pytest.mark.parametrize("name", ["G5", "A55", "GG", "AG", "5"])
def test_other_names_stay_unknown(name):
    rc, msg = _create(f"4 3 0 2 0 0\nA {name}\n1 0\n")
    assert rc == BCHK_EINVAL and "Unknown kernel" in msg


@pytest.mark.parametrize("layers,name", [("A G", "G"), ("a5 A", "a5"), ("A A5 g", "A5")])
def test_design_bec_refuses_a_named_kernel_by_name(layers, name):
    F = load()
    with pytest.raises(F.BchkError) as e:
        F.design_bec(layers, 3)
    assert f"bchk error {BCHK_EINVAL}:" in str(e.value) and f"named kernel {name}" in str(e.value)


# ------------------------------------------------------------------ GPU

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
@pytest.mark.parametrize("path,L", CASES, ids=_case_ids)
def test_gpu_decoder_matches_reference(path, L, kdir):
    fx = NL.fixture(path)
    d = load().PolarListDecoder(fx.spec, L, kernel_dir=kdir)
    assert_lists_equal(d.decode(fx.llr), fx.decoded(L), f"GPU {fx.name} L={L}")


@pytest.mark.gpu
def test_gpu_lower_case_names_decode_the_same(kdir):
    fx = fx_named("A5_G")
    d = load().PolarListDecoder(fx.spec.replace("A5 G", "a5 g"), 8, kernel_dir=kdir)
    assert_lists_equal(d.decode(fx.llr), fx.decoded(8), "GPU a5 g L=8")


@pytest.mark.gpu
@pytest.mark.parametrize("path", NAMED, ids=NL.ident)
def test_gpu_encoders_match_reference(path, kdir):
    import torch
    fx = NL.fixture(path)
    d = load().PolarListDecoder(fx.spec, 1, kernel_dir=kdir)
    np.testing.assert_array_equal(d.encode(fx.info), fx.encoded)  # bchk_polar_encode_host
    t_info = _dev(fx.info)
    t_cw = _zeros((len(fx.info), d.N), torch.uint8)
    _sync()
    d.encode_device(t_info.data_ptr(), len(fx.info), t_cw.data_ptr())
    d.sync()
    np.testing.assert_array_equal(t_cw.cpu().numpy(), fx.encoded)


@pytest.mark.gpu
@pytest.mark.parametrize("path,L", OUTER_CASES, ids=_outer_ids)
def test_gpu_outer_g_with_a_list_matches_the_matrix_form(path, L, kdir):
    """G in an outer layer, list size above 1: the product carries G's state with the path, which
    the reference does not. The recorded lists are the reference's for the matrix
    form of the code; on every kept row the set of information words and the best word agree."""
    fx = NL.fixture(path)
    d = load().PolarListDecoder(NL.named_form(fx.spec), L, kernel_dir=kdir)
    cnt, info, cw, met = d.decode(fx.llr)
    for b, (c, wi, ww, wm) in enumerate(fx.decoded(L)):
        assert cnt[b] == c, (b, cnt[b], c)
        assert {r.tobytes() for r in info[b, :c]} == {r.tobytes() for r in wi}, f"row {b}: information words"
        np.testing.assert_array_equal(info[b, 0], wi[0], err_msg=f"row {b}: best word")
        np.testing.assert_array_equal(cw[b, 0], ww[0], err_msg=f"row {b}: best codeword")


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 8])
def test_gpu_budgeted_launches_carry_the_named_state(L, kdir, monkeypatch):
    """-bch8 G with the 8 x 8 layer on the search path (BCHK_POLAR_ML=2; G stays on its f/g
    processor) and a budget of one clock tick: every search round is a suspension, and G's state
    goes through the save slot with the rest of [0, o_ph)."""
    from test_polar_budget import TINY, _decoder
    fx = fx_named("bch8_G")
    one = _decoder(monkeypatch, fx.spec, L, kdir, "0", ml=2)
    tiny = _decoder(monkeypatch, fx.spec, L, kdir, TINY, ml=2)
    want = one.decode(fx.llr)
    assert one.last_launches() == 1
    got = tiny.decode(fx.llr)
    assert tiny.last_launches() > 1
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
    assert_lists_equal(got, fx.decoded(L), f"budgeted bch8_G L={L}")


class _Frozen:
    def __init__(self, spec):
        tok = spec.split()
        N, K, _, nl, nsh, npu = (int(t) for t in tok[:6])
        U, pos = N + nsh + npu, 6 + nl + nsh + npu
        self.frozen = np.zeros(U, bool)
        for _ in range(U - K):
            w = int(tok[pos])
            self.frozen[int(tok[pos + w])] = True
            pos += 1 + w


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A_A5_A", "A_A_G", "A_G_A5_A"])
def test_gpu_genie_llrs_are_the_l1_decoders(name, kdir):
    """Both kernels run pllr::named_llrs: where the genie's decision rule gets every unfrozen
    symbol right the L = 1 decoder returns the sent word, and its metric is the float sum of the
    genie's LLRs over the contradicted frozen symbols; else the first wrong bit is the same."""
    import torch
    from genie_lib import first_wrong_unfrozen, frozen_penalty
    fx = fx_named(name)
    d = load().PolarListDecoder(fx.spec, 1, kernel_dir=kdir)
    code, B = _Frozen(fx.spec), 96
    t_llr, t_info = _zeros((B, d.N), torch.float32), _zeros((B, d.K), torch.uint8)
    t_dec, t_u = _zeros((B, d.U), torch.float32), _zeros((B, d.U), torch.uint8)
    t_err, t_soft = _zeros((d.U,), torch.int64), _zeros((d.U,), torch.int64)
    info, cw = _zeros((B, 1, d.K), torch.uint8), _zeros((B, 1, d.N), torch.uint8)
    met, cnt = _zeros((B, 1), torch.float32), _zeros((B,), torch.int32)
    _sync()
    d.generate_device(1.0, B, t_llr.data_ptr(), t_info.data_ptr(), seed=11)
    d.genie_device(t_info.data_ptr(), t_llr.data_ptr(), B, t_err.data_ptr(), t_soft.data_ptr(), t_dec.data_ptr(),
                   t_u.data_ptr())
    d.decode_device(t_llr.data_ptr(), B, info.data_ptr(), cw.data_ptr(), met.data_ptr(), cnt.data_ptr())
    d.sync()
    dec, u, sent = t_dec.cpu().numpy(), t_u.cpu().numpy(), t_info.cpu().numpy()
    info, met = info.cpu().numpy(), met.cpu().numpy()
    right = wrong = 0
    for b in range(B):
        diff = np.flatnonzero(info[b, 0] != sent[b])
        first = first_wrong_unfrozen(code, dec[b], u[b])
        assert first == (int(diff[0]) if len(diff) else None), (name, b)
        if first is None:
            right += 1
            assert met[b, 0].view(np.uint32) == frozen_penalty(code, dec[b], u[b]).view(np.uint32), (name, b)
        else:
            wrong += 1
    assert right > 0 and wrong > 0  # both branches were exercised
    # the counters are integer column sums: the same whatever the batch split
    whole = d.genie_run(1.0, 300, seed=11)
    split = d.genie_run(1.0, 300, seed=11, batch=37)
    np.testing.assert_array_equal(whole[0], split[0])
    np.testing.assert_array_equal(whole[1], split[1])
    err96 = d.genie_run(1.0, B, seed=11)[0]
    np.testing.assert_array_equal(err96, ((dec < 0) != (u != 0)).sum(axis=0).astype(np.uint64))


@pytest.mark.gpu
def test_gpu_sweep_equals_generate_decode_count_by_hand(kdir):
    import torch
    from test_polar_sim import Batch
    fx = fx_named("A_A_A_A_A_G")
    d = load().PolarListDecoder(fx.spec, 8, kernel_dir=kdir)
    words, seed = 300, 9
    recs, secs, decoded = d.sweep_device(1.0, 1.5, 2, words, 10 ** 9, seed=seed, batch=128)
    assert [r[0] for r in recs] == [1.0, 2.5] and decoded == 2 * words
    for pt, (snr, c) in enumerate(recs):
        out8 = _zeros((8,), torch.int64)
        Batch(d, snr, words, seed, word0=pt * words).count_device(0, words, out8)
        assert c == out8.cpu().numpy().tolist(), (snr, c)
        assert c[0] == words and 0 < c[6]  # raw channel errors occurred
    assert recs[0][1][1] > 0  # block errors at 1 dB


@pytest.mark.gpu
def test_gpu_design_genie_takes_the_names(kdir):
    F = load()
    spec, err, soft = F.design_genie("A A A A A G", 48, 2.0, 2000, seed=3)
    lines = spec.rstrip("\n").split("\n")
    assert lines[0] == "96 48 0 6 0 0" and lines[1] == "A A A A A G"
    frozen = [int(l.split()[1]) for l in lines[2:]]
    assert len(frozen) == 48 and frozen == sorted(set(frozen)) and all(l.startswith("1 ") for l in lines[2:])
    assert len(err) == 96 and err[frozen].sum() > err.sum() - err[frozen].sum()  # the worse half is frozen
    d = F.PolarListDecoder(spec, 8)
    info = np.random.default_rng(1).integers(0, 2, (8, 48)).astype(np.uint8)
    cw = d.encode(info)
    cnt, got, gcw, _ = d.decode(np.where(cw != 0, -8.0, 8.0).astype(np.float32))  # noiseless: bit 1 -> negative LLR
    np.testing.assert_array_equal(got[:, 0], info)
    np.testing.assert_array_equal(gcw[:, 0], cw)
    with pytest.raises(F.BchkError):
        F.design_genie("A G7", 3, 2.0, 100)
