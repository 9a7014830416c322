"""The tiered mixed-kernel SC-list decoder (csrc/polar_mixed_tiered.hip,
bchk_polar_create_tiered_mixed, PolarListDecoder(state="tiered_mixed")): polar_mixed_kernel with
the state of the layers before `split` -- LLRs, partial sums, offset states, a named layer's
carried floats -- in a device-memory workspace, shared between paths and copied on write. Its
lists must be those of the LDS mixed kernel, the C oracle and the compiled vendored library bit
for bit: count, information vectors, codewords, f32 metric bits, list order -- at every split, and
past the lengths the LDS kernel and the C oracle (U <= 4096) take, where the recorded reference
lists of tests/golden/long_mixed_ref_* (scripts/make_long_mixed_golden.py) decide.
"""
import glob
import os

import numpy as np
import pytest

from bchk_pkg import load
from polar_lib import PolarOracle, arikan_spec, awgn_llr
from polar_ref_lib import GOLD, load_fixture
from test_polar_mixed import KERNELS, kdir, mixed_spec  # noqa: F401  (kdir: the kernel files' fixture)
from test_polar_sclist import assert_same, workload

NAMED = {"A": 2, "G": 3, "A5": 5}


def tm(spec, L, kdir=None, split=None):
    return load().PolarListDecoder(spec, L, kernel_dir=kdir, state="tiered_mixed", split=split)


def lds(spec, L, kdir=None):
    return load().PolarListDecoder(spec, L, kernel_dir=kdir)


def any_spec(layers, K, dyn=0, punct=(), seed=0):
    """mixed_spec over kernel files and the named kernels G / A5 too."""
    if all(n == "A" or n in KERNELS for n in layers):
        return mixed_spec(layers, K, dyn, punct, seed)
    sizes = [NAMED[n] if n in NAMED else len(KERNELS[n]) for n in layers]
    U = int(np.prod(sizes))
    rng = np.random.default_rng(seed)
    order = list(range(U))
    for _ in range(U // 8):
        i = int(rng.integers(max(0, U - K - 4), min(U, U - K + 4)))
        j = int(rng.integers(max(0, U - K - 4), min(U, U - K + 4)))
        order[i], order[j] = order[j], order[i]
    frozen = sorted(order[:U - K])
    cand = [f for f in frozen if f >= 2]
    dynset = set(rng.choice(cand, size=min(dyn, len(cand)), replace=False).tolist()) if dyn else set()
    lines = [f"{U - len(punct)} {K} 0 {len(layers)} 0 {len(punct)}",
             " ".join(n if n in NAMED else f"-{n}.txt" for n in layers)]
    if punct:
        lines.append(" ".join(str(p) for p in punct))
    for f in frozen:
        if f in dynset:
            a, b = sorted(rng.choice(f, size=2, replace=False).tolist())
            lines.append(f"3 {a} {b} {f}")
        else:
            lines.append(f"1 {f}")
    return "\n".join(lines) + "\n"


def words(o, K, B, snr, seed):
    info = np.random.default_rng(seed).integers(0, 2, (B, K)).astype(np.uint8)
    return awgn_llr(o.encode(info), snr, K / o.N, seed=seed + 1)


class LdsReference:
    """The C oracle restates neither G nor A5 (oracle/polar_oracle.c), so a code with a named layer
    has the LDS mixed kernel as its reference here -- itself pinned to the compiled vendored library
    by tests/test_polar_named_kernels.py -- and the recorded lists of tests/golden/named_ref_*
    below."""

    def __init__(self, spec, kdir):
        self.spec, self.kdir = spec, kdir
        d = lds(spec, 1, kdir)
        self.N, self.K, self.U, self.encode = d.N, d.K, d.U, d.encode

    def decode_batch(self, llr, L):
        return lds(self.spec, L, self.kdir).decode(llr)


def reference(spec, kdir):
    named = any(n in NAMED and n != "A" for n in spec.split("\n")[1].split())
    return LdsReference(spec, kdir) if named else PolarOracle(spec, kdir)


EBCH3 = (("bch16", "bch16", "bch16"), 2048)  # U = 4096: 139 KB of LDS at L = 8, refused at 16
A4EBCH2 = (("A", "A", "A", "A", "bch16", "bch16"), 2048)  # U = 4096: refused by the LDS state at L = 8


# ---------------------------------------------------------------- host side (no GPU needed)

def test_tiered_mixed_takes_a_code_past_the_lds_limit(kdir):
    """eBCH16^3 at L = 16: state="lds" refuses it; the new state passes every spec and limit
    check, so what is left to fail is the missing device."""
    import torch
    spec = mixed_spec(EBCH3[0], EBCH3[1], 4, (), seed=3)
    with pytest.raises(load().BchkError, match="LDS"):
        lds(spec, 16, kdir)
    if torch.cuda.is_available():
        d = tm(spec, 16, kdir)
        assert 1 <= d.split <= 3 and d.state_info()["lds_bytes"] <= 160 * 1024
        d.close()
    else:
        with pytest.raises(load().BchkError, match="device|HIP"):
            tm(spec, 16, kdir)


def test_tiered_mixed_refusals(kdir):
    F = load()
    with pytest.raises(F.BchkError, match="search layer"):  # the 64 x 64 kernel stays on the LDS state
        tm(mixed_spec(("bch64", "A"), 64, 0, (), seed=1), 4, kdir)
    small = mixed_spec(("k3", "A", "k4"), 12, 2, (), seed=2)
    for split in (0, 4, -2):
        with pytest.raises(F.BchkError, match="split -?[0-9]+ out of range"):
            tm(small, 4, kdir, split=split)
    with pytest.raises(ValueError, match="split"):
        F.PolarListDecoder(small, 4, kernel_dir=kdir, state="lds", split=2)
    with pytest.raises(F.BchkError, match="tiered state is built for all-Arikan codes"):
        F.PolarListDecoder(small, 4, kernel_dir=kdir, state="tiered")
    with pytest.raises(F.BchkError, match="still needs [0-9]+ B of LDS"):  # 32 paths of the U = 2048 sub-code stay in LDS
        tm(mixed_spec(A4EBCH2[0], A4EBCH2[1], 4, (), seed=3), 32, kdir, split=1)
    with pytest.raises(F.BchkError, match="list size"):
        tm(small, 33, kdir)


LONG = sorted(glob.glob(os.path.join(GOLD, "long_mixed_ref_*.txt.gz")))


def test_long_mixed_fixtures_are_present():
    assert len(LONG) == 2


# ---------------------------------------------------------------- GPU parity

CODES = [  # layers, K, dynamic constraints, punctured positions
    (("A", "k4", "A"), 8, 0, ()),            # U = 16
    (("k3", "A", "k4"), 12, 2, (5,)),        # U = 24, odd sizes
    (("A", "A", "bch8"), 16, 3, ()),         # U = 32: enumeration innermost
    (("bch8", "A", "A"), 16, 2, (3, 9)),     # ... and on the channel side
    (("k4", "bch8"), 16, 2, ()),
    (("A", "bch16", "A"), 32, 4, ()),        # U = 64, the trellis between Arikan layers
    (("bch16", "k4"), 32, 2, ()),
    (("G", "A", "A5"), 15, 2, ()),           # U = 30: named layers on either side
    (("A5", "G", "A"), 15, 0, (4,)),
]


def check_every_split(spec, kdir, L, B, snr, seed):
    o = reference(spec, kdir)
    llr = words(o, o.K, B, snr, seed)
    want = o.decode_batch(llr, L)
    assert_same(lds(spec, L, kdir).decode(llr), want)
    nl = int(spec.split()[3])
    for split in range(1, nl + 1):
        d = tm(spec, L, kdir, split)
        assert d.split == split
        got = d.decode(llr)
        d.close()
        assert_same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("layers,K,dyn,punct", CODES, ids=["-".join(c[0]) for c in CODES])
@pytest.mark.parametrize("L", [1, 2, 4, 8, 32])
def test_gpu_tiered_mixed_every_split(kdir, layers, K, dyn, punct, L):
    """An Arikan, enumeration, trellis or named layer on either side of every boundary."""
    spec = any_spec(layers, K, dyn, punct, seed=len(layers) * 11 + K)
    check_every_split(spec, kdir, L, 64 if L == 32 else 96, 1.5, seed=K + L)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [4, 32])
def test_gpu_tiered_mixed_8x8_through_the_trellis(kdir, L, monkeypatch):
    monkeypatch.setenv("BCHK_POLAR_TRELLIS", "8")
    spec = mixed_spec(("A", "bch8", "A"), 16, 2, (3,), seed=19)
    check_every_split(spec, kdir, L, 64, 1.0, seed=40 + L)


@pytest.mark.gpu
@pytest.mark.parametrize("layers,K", [(("A", "bch8", "A"), 16), (("A5", "G", "A"), 15)], ids=["matrix", "named"])
def test_gpu_tiered_mixed_ties_and_zeros(kdir, layers, K):
    """Equal metrics and zero LLRs: only path indices may break ties, never array indices."""
    spec = any_spec(layers, K, 2, (), seed=7)
    o = reference(spec, kdir)
    q = (4.0 * np.round(words(o, K, 96, 1.0, seed=77) / 4.0)).astype(np.float32)
    assert np.any(q == 0)
    want = o.decode_batch(q, 8)
    assert_same(lds(spec, 8, kdir).decode(q), want)
    for split in (1, 2, 3):
        assert_same(tm(spec, 8, kdir, split).decode(q), want)


@pytest.mark.gpu
def test_gpu_tiered_mixed_full_lists(kdir):
    """L = 2^K keeps every codeword: every unfrozen phase clones, later ones kill too."""
    for layers, K in ((("k3", "A"), 3), (("A", "G", "A"), 5)):
        spec = any_spec(layers, K, 0, (), seed=K)
        o = reference(spec, kdir)
        llr = words(o, K, 40, 0.0, seed=K)
        for split in (1, len(layers)):
            got = tm(spec, 1 << K, kdir, split).decode(llr)
            assert np.all(got[0] == 1 << K)
            assert_same(got, o.decode_batch(llr, 1 << K))


@pytest.mark.gpu
def test_gpu_tiered_mixed_state_reuse_across_codewords(kdir, monkeypatch):
    """Three waves decode 1000 codewords each: nothing of a codeword's arrays or indices may
    reach the next."""
    monkeypatch.setenv("BCHK_POLAR_GRID", "3")
    spec = mixed_spec(("k3", "A", "k4"), 12, 2, (5,), seed=45)
    o = PolarOracle(spec, kdir)
    llr = words(o, 12, 3000, 2.0, seed=21)
    d = tm(spec, 8, kdir, 3)
    assert d.state_info()["grid"] == 3
    assert_same(d.decode(llr), o.decode_batch(llr, 8))


# (layers, K, L, split asked) -> (split, lds_bytes, workspace_bytes) of state_info(), read off the
# library of commit b2bf5e7 on an MI355X (not computed by the code under test). With split=None
# A^4 x eBCH16^2 at L = 32 does not fit LDS at splits 1 and 2 (the rule's first loop), and it and
# three other codes then move further layers out for more waves per CU (the second loop).
B16 = "bch16"
AUTO_CHOICE = {
    ((B16, B16, B16), 2048, 8, None): (1, 18864, 122880), ((B16, B16, B16), 2048, 8, 3): (3, 13888, 128000),
    ((B16, B16, B16), 2048, 16, None): (2, 16752, 238592), ((B16, B16, B16), 2048, 16, 1): (1, 25952, 229376),
    (("A", B16, B16, B16), 4096, 8, None): (3, 25024, 373248), (("A", B16, B16, B16), 4096, 8, 2): (2, 29632, 368640),
    (A4EBCH2[0], 2048, 8, None): (4, 20432, 233472), (A4EBCH2[0], 2048, 8, 6): (6, 15456, 238592),
    (("bch8", "A5", "A", "k4"), 160, 8, None): (1, 4944, 10240), (("bch8", "A5", "A", "k4"), 160, 8, 3): (3, 3296, 12032),
    (A4EBCH2[0], 2048, 32, None): (5, 23360, 903168), (A4EBCH2[0], 2048, 32, 3): (3, 90880, 835584),
}


@pytest.mark.gpu
def test_tiered_auto_choice_pinned(kdir):
    """What split=None chooses, and the layout sizes at it and at one explicit split: creation
    only, nothing is decoded. grid is left out (it follows the CU count and BCHK_POLAR_WORKSPACE_MB)."""
    for (layers, K, L, ask), want in AUTO_CHOICE.items():
        d = tm(any_spec(layers, K, 0, (), seed=1), L, kdir, ask)
        st = d.state_info()
        d.close()
        assert (st["split"], st["lds_bytes"], st["workspace_bytes"]) == want, (layers, L, ask)


@pytest.mark.gpu
def test_gpu_tiered_mixed_all_arikan_cross_check():
    """An all-Arikan code through this kernel: the lists of the Arikan tiered and LDS kernels."""
    spec, o, info, llr = workload(7, 64, 8, (0, 3), 2.0, 96, seed=5)
    F = load()
    want = F.PolarListDecoder(spec, 8).decode(llr)
    assert_same(want, o.decode_batch(llr, 8))
    assert_same(F.PolarListDecoder(spec, 8, state="tiered", split=3).decode(llr), want)
    for split in (1, 4, 7):
        assert_same(tm(spec, 8, split=split).decode(llr), want)


@pytest.mark.gpu
@pytest.mark.parametrize("layers,K,L", [EBCH3 + (16,), A4EBCH2 + (8,)], ids=["ebch16x3-L16", "A4-ebch16x2-L8"])
def test_gpu_tiered_mixed_past_the_lds_limit(kdir, layers, K, L):
    spec = mixed_spec(layers, K, 4, (), seed=3)
    with pytest.raises(load().BchkError, match="LDS"):
        lds(spec, L, kdir)
    o = PolarOracle(spec, kdir)
    llr = words(o, K, 3, 2.0, seed=L)
    assert_same(tm(spec, L, kdir).decode(llr), o.decode_batch(llr, L))


@pytest.mark.gpu
@pytest.mark.parametrize("path", LONG, ids=[os.path.basename(p)[15:-7] for p in LONG])
def test_gpu_tiered_mixed_matches_recorded_reference(path, tmp_path):
    """Past the C oracle (U > 4096): the recorded lists of the compiled vendored library."""
    fx = load_fixture(path)
    fx.write_kernels(str(tmp_path))
    llr = fx.llr
    for L in fx.list_sizes:
        cnt, info, cw, met = tm(fx.spec, L, str(tmp_path)).decode(llr)
        for b, (c, winfo, wcw, wmet) in enumerate(fx.decoded(L)):
            assert cnt[b] == c, f"row {b}"
            np.testing.assert_array_equal(info[b, :c], winfo, err_msg=f"info, row {b}")
            np.testing.assert_array_equal(cw[b, :c], wcw, err_msg=f"codewords, row {b}")
            np.testing.assert_array_equal(met[b, :c].view(np.uint32), wmet, err_msg=f"metrics, row {b}")


def _named_cases():
    import named_lib as NL
    return [(p, L) for p in NL.named_files() for L in NL.fixture(p).list_sizes if NL.fixture(p).has("decode")]


@pytest.mark.gpu
@pytest.mark.parametrize("path,L", _named_cases(), ids=lambda v: os.path.basename(v)[10:-7] if isinstance(v, str) else f"L{v}")
def test_gpu_tiered_mixed_matches_recorded_named_lists(path, L, tmp_path):
    """G and A5 at every split against the reference's own recorded lists."""
    fx = load_fixture(path)
    fx.write_kernels(str(tmp_path))
    want = fx.decoded(L)
    for split in range(1, int(fx.spec.split()[3]) + 1):
        cnt, info, cw, met = tm(fx.spec, L, str(tmp_path), split).decode(fx.llr)
        for b, (c, winfo, wcw, wmet) in enumerate(want):
            assert cnt[b] == c, f"split {split} row {b}"
            np.testing.assert_array_equal(info[b, :c], winfo, err_msg=f"info, split {split} row {b}")
            np.testing.assert_array_equal(cw[b, :c], wcw, err_msg=f"codewords, split {split} row {b}")
            np.testing.assert_array_equal(met[b, :c].view(np.uint32), wmet, err_msg=f"metrics, split {split} row {b}")


@pytest.mark.gpu
def test_gpu_tiered_mixed_sweep(kdir):
    import torch
    from test_polar_sim import Batch, _sync, _zeros
    spec = mixed_spec(("A", "bch8", "A"), 16, 2, (), seed=8)
    a = tm(spec, 4, kdir).sweep_device(1.0, 1.0, 2, 2000, 20, seed=3)
    b = lds(spec, 4, kdir).sweep_device(1.0, 1.0, 2, 2000, 20, seed=3)
    assert a[0] == b[0] and a[2] == b[2]
    # a code only the new state takes: one point against its three steps done by hand
    d = tm(mixed_spec(EBCH3[0], EBCH3[1], 4, (), seed=3), 16, kdir)
    (pt,), _, nwords = d.sweep_device(2.0, 1.0, 1, 32, 1 << 40, seed=5)
    assert nwords == 32
    out8 = _zeros((8,), torch.int64)
    _sync()
    Batch(d, 2.0, 32, 5).count_device(0, 32, out8)
    assert pt[1] == [int(v) for v in out8.cpu().numpy()]
    assert pt[1][0] == 32


@pytest.mark.gpu
def test_gpu_tiered_mixed_workspace_and_caller_stream(kdir):
    import torch
    layers, L, split = ("bch8", "A5", "A", "k4"), 8, 3
    spec = any_spec(layers, 160, 6, (), seed=31)
    o = reference(spec, kdir)
    U = o.U
    assert U == 320
    llr = words(o, o.K, 200, 2.0, seed=31)
    d = tm(spec, L, kdir, split)
    st = d.state_info()
    # the mapped channel row, C_0 of L paths, and per layer before the split L arrays of S_{j+1}
    # (floats), C_{j+1} (l outer[j+1] bytes) and the layer's state: a matrix layer's offsets (as
    # many bytes again), A5's three floats and one byte per element
    per_wg, outer = 4 * U + L * U, U
    for name in layers[:split]:
        l = NAMED[name] if name in NAMED else len(KERNELS[name])
        outer //= l
        state = {"A": 0, "A5": 13 * outer, "G": 4 * outer}.get(name, l * outer)
        per_wg += L * (4 * outer + l * outer + state)
    assert st["workspace_bytes"] >= per_wg and st["grid"] >= 1 and st["split"] == split
    assert d.scratch_bytes()[0] >= st["grid"] * per_wg
    want = d.decode(llr)
    assert_same(want, o.decode_batch(llr, L))
    dev = torch.device("cuda:0")
    t_llr = torch.from_numpy(llr).to(dev)
    t_info = torch.zeros((200, L, o.K), dtype=torch.uint8, device=dev)
    t_cw = torch.zeros((200, L, o.N), dtype=torch.uint8, device=dev)
    t_met = torch.zeros((200, L), dtype=torch.float32, device=dev)
    t_cnt = torch.zeros(200, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    d.decode_device(t_llr.data_ptr(), 200, t_info.data_ptr(), t_cw.data_ptr(), t_met.data_ptr(), t_cnt.data_ptr(),
                    stream=s.cuda_stream)
    s.synchronize()
    assert_same((t_cnt.cpu().numpy(), t_info.cpu().numpy(), t_cw.cpu().numpy(), t_met.cpu().numpy()), want)
