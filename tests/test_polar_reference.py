"""The polar half pinned to THE REFERENCE ITSELF: tests/golden/polar_ref_*.txt.gz hold inputs and
the recorded outputs of the reference's vendored library (CMixedKernelListDecoder::Decode,
CMixedKernelEncoder::Encode, CTrellisKernelProcessor::GetLLRs), compiled as it stands into
oracle/_ref/polar_ref (oracle/Makefile, oracle/polar_ref.cpp) and run by `python
oracle/make_golden.py polar`. Format: tests/polar_ref_lib.py.

  CPU   oracle/polar_oracle.c against every fixture: list count, information vectors,
        codewords, list order and f32 metric bits; its trellis / enumeration / ordered-
        statistics kernel LLRs against the trellis fixtures as f32 bits; its encoder.
  GPU   PolarListDecoder.decode / .encode (csrc/polar_sclist.hip for Arikan codes,
        csrc/polar_mixed.hip for matrix kernels) against the same fixtures, directly.
  regeneration: where oracle/_ref/polar_ref exists, re-running it on a fixture's inputs gives
        the fixture byte for byte.

The dyn_* fixtures (tests/dense_codes.py) are codes with 33 to 64 dynamic freezing constraints
live at once and constraints of 65 and 130 terms: the upper half of the decoders' 64-bit mask.
The lists_* fixtures (`oracle/make_golden.py polar-lists`) record four codes at the list sizes
3, 5, 6, 7, 12, 24 and 31, none a power of two (tests/test_polar_list_sizes.py).

Not pinned (no fixture can exist): kernels of size >= 64, which the reference's trellis
processor refuses (TrellisKernelProcessor.cpp:71-72) -- the 64 x 64 ordered-statistics path
stays checked against the oracle's enumeration properties only (tests/test_polar_ml.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

import polar_ref_lib as R
from bchk_pkg import load
from polar_lib import PolarOracle
from polar_lib import lib as plib

CODE_FILES = R.fixture_files("code")
TRELLIS_FILES = R.fixture_files("trellis")
_ids = lambda p: os.path.basename(p)[len("polar_ref_"):-len(".txt.gz")]  # noqa: E731

_fx = {}


def fixture(path):
    if path not in _fx:
        _fx[path] = R.load_fixture(path)
    return _fx[path]


@pytest.fixture(scope="module")
def kdir(tmp_path_factory):
    """Every kernel file of every fixture (the same name always holds the same matrix)."""
    d = tmp_path_factory.mktemp("ref_kernels")
    seen = {}
    for p in CODE_FILES + TRELLIS_FILES:
        for fname, K in fixture(p).kernels.items():
            assert fname not in seen or np.array_equal(seen[fname], K)
            seen[fname] = K
        fixture(p).write_kernels(str(d))
    return str(d)


CASES = [(p, L) for p in CODE_FILES for L in fixture(p).list_sizes]
_case_ids = [f"{_ids(p)}-L{L}" for p, L in CASES]


def assert_lists_equal(got, want, what):
    """got: (count [B], info [B][L][K], cw [B][L][N], metric f32 [B][L]); want: Fixture.decoded."""
    cnt, info, cw, met = got
    assert len(cnt) == len(want)
    for b, (c, wi, ww, wm) in enumerate(want):
        assert cnt[b] == c, f"{what}: list count, row {b}: {cnt[b]} != {c}"
        np.testing.assert_array_equal(info[b, :c], wi, err_msg=f"{what}: information vectors, row {b}")
        np.testing.assert_array_equal(cw[b, :c], ww, err_msg=f"{what}: codewords, row {b}")
        np.testing.assert_array_equal(np.ascontiguousarray(met[b, :c]).view(np.uint32), wm,
                                      err_msg=f"{what}: metric bits, row {b}")


# ------------------------------------------------------------------ the fixtures themselves

def test_the_fixture_set_is_the_one_the_generator_writes():
    names = sorted(_ids(p) for p in CODE_FILES + TRELLIS_FILES)
    assert names == sorted([
        "arikan_n3", "arikan_n4", "arikan_n5", "arikan_n6", "arikan_n8", "arikan_n7_ties",
        "mixed_k4_A", "mixed_bch8_A", "mixed_bch16_A", "mixed_bch32f", "mixed_bch32f_A",
        "short_arikan_n6", "short_bch16_A", "short_arikan_n7",
        "dyn_arikan_n8_a64", "dyn_arikan_n7_a33", "dyn_A_bch16_bch8_a40",
        "lists_arikan_n6", "lists_arikan_n7_ties", "lists_bch8_A", "lists_dyn_arikan_n7_a33",
        "trellis_bch8", "trellis_bch16", "trellis_bch32", "trellis_bch32f"])
    for p in CODE_FILES:
        fx = fixture(p)
        if fx.name.startswith("lists"):  # list sizes that are no power of two (tests/test_polar_list_sizes.py)
            assert fx.list_sizes == [3, 5, 6, 7, 12, 24, 31] and len(fx.info) == 30
            assert len(fx.llr) == (28 if fx.name == "lists_dyn_arikan_n7_a33" else 32)  # words dropped for the file's size
            continue
        want = [8] if fx.name.endswith("ties") else [1, 4, 8] if fx.name.startswith(("mixed", "short", "dyn")) else [1, 2, 4, 8, 32]
        assert fx.list_sizes == want and 32 <= len(fx.llr) <= 64 and len(fx.info) == 30


def test_fixtures_exercise_what_they_are_for():
    """Lists really diverge; the full lists are full; the tie fixture has equal metrics inside
    a list and exact-zero LLRs; punctured / dynamic-frozen codes are what the names say."""
    for p in CODE_FILES:
        fx = fixture(p)
        L = max(fx.list_sizes)
        rows = fx.decoded(L)
        assert all(c >= 1 for c, *_ in rows) and max(c for c, *_ in rows) > 1
        assert any(len(set(m.tolist())) > 1 for _, _, _, m in rows)
    for name, K in (("arikan_n3", 3), ("arikan_n4", 5)):
        fx = fixture(os.path.join(R.GOLD, f"polar_ref_{name}.txt.gz"))
        assert all(c == 1 << K for c, *_ in fx.decoded(1 << K))
    t = fixture(os.path.join(R.GOLD, "polar_ref_arikan_n7_ties.txt.gz"))
    assert np.all(t.llr % 4 == 0) and np.any(t.llr == 0)
    assert any(len(set(m.tolist())) < len(m) for _, _, _, m in t.decoded(8))
    assert fixture(os.path.join(R.GOLD, "polar_ref_arikan_n6.txt.gz")).spec.split("\n")[2] == "1 7"
    assert fixture(os.path.join(R.GOLD, "polar_ref_arikan_n8.txt.gz")).spec.count("\n3 ") == 12
    assert fixture(os.path.join(R.GOLD, "polar_ref_arikan_n5.txt.gz")).spec.count("\n3 ") == 3
    # dense dynamic freezing: as many constraints live at once as the name says, and every bit of
    # the mask's upper half that the code uses carries a 1 in some transmitted word -- the frozen
    # symbol on that bit, the XOR of its listed terms over the fixture's information words
    import dense_codes
    from polar_lib import constraint_bits, max_active, spec_inputs
    assert sorted(dense_codes.FIXTURES) == sorted(_ids(p) for p in CODE_FILES if _ids(p).startswith("dyn"))
    for name in dense_codes.FIXTURES:
        fx = fixture(os.path.join(R.GOLD, f"polar_ref_{name}.txt.gz"))
        assert fx.spec == dense_codes.spec(name)
        active = dense_codes.claimed_active(name)
        assert max_active(fx.spec) == active > 32
        bit = constraint_bits(fx.spec)
        assert max(bit.values()) == active - 1
        u = spec_inputs(fx.spec, len(fx.encoded[0]), fx.info)
        for b in range(32, active):
            assert any(u[:, f].any() for f, v in bit.items() if v == b), (name, b)


def test_fixture_kernels_are_the_products_extended_bch_kernels():
    F = load()
    for p in CODE_FILES + TRELLIS_FILES:
        for fname, K in fixture(p).kernels.items():
            if fname.startswith("bch"):
                power = {8: 3, 16: 4, 32: 5}[len(K)]
                want = F.kernel_ebch(power)
                if fname == "bch32f.txt":
                    want = F.kernel_field_order(power, want)
                np.testing.assert_array_equal(K, want, err_msg=fname)


# ------------------------------------------------------------------ CPU: the oracle

@pytest.mark.parametrize("path,L", CASES, ids=_case_ids)
def test_oracle_decoder_matches_reference(path, L, kdir):
    fx = fixture(path)
    o = PolarOracle(fx.spec, kdir)
    assert_lists_equal(o.decode_batch(fx.llr, L), fx.decoded(L), f"oracle {fx.name} L={L}")


@pytest.mark.parametrize("path", CODE_FILES, ids=_ids)
def test_oracle_encoder_matches_reference(path, kdir):
    fx = fixture(path)
    np.testing.assert_array_equal(PolarOracle(fx.spec, kdir).encode(fx.info), fx.encoded)


class _PlrKernel(C.Structure):
    _fields_ = [("size", C.c_int), ("arikan", C.c_int), ("K", C.c_uint8 * 4096), ("Kinv", C.c_uint8 * 4096)]


PLR_BY_ENUM, PLR_BY_TRELLIS, PLR_BY_ML = 0, 1, 2


@pytest.mark.parametrize("path", TRELLIS_FILES, ids=_ids)
def test_oracle_kernel_llrs_match_reference_trellis_processor(path):
    """Every phase, the known inputs' rows applied as sign flips (GetLLRs :246-267), through
    the oracle's dispatcher and through each of its three methods where the coset allows
    (enumeration up to 2^16 words), as f32 bits."""
    fx = fixture(path)
    lib = plib()
    lib.plr_minsum_llr.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.plr_minsum_llr.restype = C.c_float
    lib.plr_minsum_llr_by.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.plr_minsum_llr_by.restype = C.c_float
    (K,) = fx.kernels.values()
    l = len(K)
    k = _PlrKernel()
    k.size, k.arikan = l, 0
    for i, v in enumerate(K.ravel()):
        k.K[i] = int(v)
    want = [np.array([int(w, 16) for w in r.split()], np.uint32) for r in fx.get("trellis_out")]
    assert len(want) == 16
    for row, w in zip(fx.get("trellis_in"), want):
        ub, *yh = row.split()
        u = R.bits(ub)
        y = np.array([int(h, 16) for h in yh], np.uint32).view(np.float32)
        off = np.zeros(l, np.uint8)
        for ph in range(l):
            if ph and u[ph - 1]:
                off ^= K[ph - 1]
            ys = np.where(off != 0, -y, y).astype(np.float32)
            yp = ys.ctypes.data_as(C.c_void_p)
            got = {"default": lib.plr_minsum_llr(C.byref(k), ph, yp),
                   "trellis": lib.plr_minsum_llr_by(C.byref(k), ph, yp, PLR_BY_TRELLIS),
                   "ml": lib.plr_minsum_llr_by(C.byref(k), ph, yp, PLR_BY_ML)}
            if l - ph - 1 <= 16:
                got["enum"] = lib.plr_minsum_llr_by(C.byref(k), ph, yp, PLR_BY_ENUM)
            for how, g in got.items():
                assert np.float32(g).view(np.uint32) == w[ph], (fx.name, ph, how, g, w[ph])


@pytest.mark.parametrize("path", CODE_FILES + TRELLIS_FILES, ids=_ids)
def test_fixture_regenerates_byte_for_byte(path, tmp_path):
    if not os.path.exists(R.POLAR_REF):
        pytest.skip("oracle/_ref/polar_ref is not built (the reference tree is absent)")
    fx = fixture(path)
    again = R.regenerate(fx, str(tmp_path))
    assert again.dumps() == fx.dumps()
    out = tmp_path / "again.txt.gz"
    again.save(str(out))
    assert out.read_bytes() == open(path, "rb").read()


# ------------------------------------------------------------------ GPU: the product, directly

@pytest.mark.gpu
@pytest.mark.parametrize("path,L", CASES, ids=_case_ids)
def test_gpu_decoder_matches_reference(path, L, kdir):
    fx = fixture(path)
    d = load().PolarListDecoder(fx.spec, L, kernel_dir=kdir)
    assert_lists_equal(d.decode(fx.llr), fx.decoded(L), f"GPU {fx.name} L={L}")


@pytest.mark.gpu
@pytest.mark.parametrize("path,L", [c for c in CASES if _ids(c[0]).startswith("mixed")],
                         ids=[i for i in _case_ids if i.startswith("mixed")])
def test_gpu_mixed_decoder_trellis_everywhere_matches_reference(path, L, kdir, monkeypatch):
    """Every matrix layer through the GPU's trellis (BCHK_POLAR_TRELLIS=2) instead of its coset
    enumeration."""
    monkeypatch.setenv("BCHK_POLAR_TRELLIS", "2")
    fx = fixture(path)
    d = load().PolarListDecoder(fx.spec, L, kernel_dir=kdir)
    assert_lists_equal(d.decode(fx.llr), fx.decoded(L), f"GPU trellis {fx.name} L={L}")


@pytest.mark.gpu
@pytest.mark.parametrize("path", CODE_FILES, ids=_ids)
def test_gpu_encoder_matches_reference(path, kdir):
    fx = fixture(path)
    d = load().PolarListDecoder(fx.spec, 1, kernel_dir=kdir)
    np.testing.assert_array_equal(d.encode(fx.info), fx.encoded)  # host side (polar_host.cpp)
    # and the encoder kernel (csrc/polar_enc_device.h)
    import torch
    dev = torch.device("cuda:0")
    t_info = torch.from_numpy(fx.info).to(dev)
    t_cw = torch.zeros((len(fx.info), d.N), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    d.encode_device(t_info.data_ptr(), len(fx.info), t_cw.data_ptr())
    d.sync()
    np.testing.assert_array_equal(t_cw.cpu().numpy(), fx.encoded)
