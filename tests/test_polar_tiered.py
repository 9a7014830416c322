"""The tiered SC-list decoder (csrc/polar_sclist_tiered.hip, bchk_polar_create_tiered,
PolarListDecoder(state="tiered")): the all-Arikan list decoder with the layers 1..split of
every path in a device-memory workspace, shared between paths and copied on write. Its lists
must be those of the LDS kernel, the C oracle and the compiled vendored library bit for bit:
count, information vectors, codewords, f32 metric bits, list order -- at every split, and past
the lengths the LDS kernel (U L <~ 36000) and the C oracle (U <= 4096) take, where the
recorded reference lists of tests/golden/long_ref_* (scripts/make_long_golden.py) decide.
"""
import glob
import os

import numpy as np
import pytest

from bchk_pkg import load
from polar_lib import PolarOracle, arikan_spec, awgn_llr
from polar_ref_lib import GOLD, load_fixture
from test_polar_sclist import assert_same, gpu_decoder, workload


def tiered(spec, L, split=None):
    return load().PolarListDecoder(spec, L, state="tiered", split=split)


# ---------------------------------------------------------------- host side (no GPU needed)

def test_tiered_takes_a_code_past_the_lds_limit():
    """(2048, 1024) at L = 32 is refused with state="lds" (test_polar_sclist); the tiered state
    passes every spec and limit check, so what is left to fail is the missing device."""
    import torch
    spec = arikan_spec(11, 1024)
    if torch.cuda.is_available():
        d = tiered(spec, 32)
        assert 1 <= d.split <= 11 and d.state_info()["lds_bytes"] <= 160 * 1024
        d.close()
    else:
        with pytest.raises(load().BchkError, match="device|HIP"):
            tiered(spec, 32)


def test_tiered_refusals(tmp_path):
    F = load()
    (tmp_path / "k2.txt").write_text("2\n1 0\n1 1\n")
    frozen3 = "1 0\n1 1\n1 2\n"
    for spec, kdir in (("6 3 0 2 0 0\nG A\n" + frozen3, None), ("4 1 0 2 0 0\n-k2.txt A\n" + frozen3, str(tmp_path))):
        with pytest.raises(F.BchkError, match="tiered state is built for all-Arikan codes"):
            F.PolarListDecoder(spec, 4, kernel_dir=kdir, state="tiered")
    for split in (0, 6, -2):
        with pytest.raises(F.BchkError, match="split -?[0-9]+ out of range"):
            tiered(arikan_spec(5, 16), 4, split=split)
    with pytest.raises(F.BchkError, match="LDS"):  # 32 paths of 8192 floats each stay in LDS
        tiered(arikan_spec(14, 8192), 32, split=1)
    with pytest.raises(F.BchkError, match="layers unsupported|exceeds 16384"):
        tiered(arikan_spec(15, 16384), 2)
    with pytest.raises(F.BchkError, match="list size"):
        tiered(arikan_spec(5, 16), 33)
    with pytest.raises(ValueError, match="split"):
        F.PolarListDecoder(arikan_spec(5, 16), 4, state="lds", split=2)
    with pytest.raises(ValueError, match="state"):
        F.PolarListDecoder(arikan_spec(5, 16), 4, state="hbm")


# ---------------------------------------------------------------- GPU parity

SMALL = [  # n, K, dynamic constraints, punctured positions
    (3, 4, 0, ()),
    (5, 16, 3, ()),
    (6, 32, 5, (1, 7)),
    (7, 64, 8, ()),
    (8, 128, 12, (0, 3, 17, 40)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,dyn,punct", SMALL)
@pytest.mark.parametrize("L", [1, 2, 4, 8, 32])
def test_gpu_tiered_every_split(n, K, dyn, punct, L):
    """Every boundary 1..n: n >= 6 has sub-word and whole-word packed-C butterflies on each side."""
    spec, o, info, llr = workload(n, K, dyn, punct, 1.0 + 0.25 * n, 96, seed=n * 7 + L)
    want = o.decode_batch(llr, L)
    assert_same(gpu_decoder(spec, L).decode(llr), want)
    for split in range(1, n + 1):
        d = tiered(spec, L, split)
        assert d.split == split
        got = d.decode(llr)
        d.close()
        assert_same(got, want)


@pytest.mark.gpu
def test_gpu_tiered_ties_and_zeros():
    """Equal metrics and zero LLRs: only path indices may break ties, never array indices."""
    spec, o, info, llr = workload(7, 64, 4, (), 1.0, 96, seed=77)
    q = np.round(llr / 4.0).astype(np.float32)
    want = o.decode_batch(q, 8)
    for split in (1, 3, 7):
        assert_same(tiered(spec, 8, split).decode(q), want)


@pytest.mark.gpu
def test_gpu_tiered_full_lists():
    """L = 2^K keeps every codeword: every unfrozen phase clones, later ones kill too."""
    for n, K in ((3, 3), (4, 5)):
        spec, o, info, llr = workload(n, K, 0, (), 0.0, 40, seed=n)
        got = tiered(spec, 1 << K, n).decode(llr)
        assert np.all(got[0] == 1 << K)
        assert_same(got, o.decode_batch(llr, 1 << K))


@pytest.mark.gpu
def test_gpu_tiered_state_reuse_across_codewords(monkeypatch):
    """Three waves decode 1000 codewords each: nothing of a codeword's arrays or indices may
    reach the next."""
    monkeypatch.setenv("BCHK_POLAR_GRID", "3")
    spec, o, info, llr = workload(6, 32, 5, (1, 7), 2.0, 3000, seed=21)
    d = tiered(spec, 8, 6)
    assert d.state_info()["grid"] == 3
    assert_same(d.decode(llr), o.decode_batch(llr, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,L", [(11, 1024, 32), (12, 2048, 16), (12, 2048, 32)])
def test_gpu_tiered_past_the_lds_limit(n, K, L):
    with pytest.raises(load().BchkError, match="LDS"):
        load().PolarListDecoder(arikan_spec(n, K, dyn=8, seed=n), L)
    spec, o, info, llr = workload(n, K, 8, (), 1.5, 8, seed=n + L)
    assert_same(tiered(spec, L).decode(llr), o.decode_batch(llr, L))


# (n, L, split asked) -> (split, lds_bytes, workspace_bytes) of state_info(), read off the library
# of commit b2bf5e7 on an MI355X (not computed by the code under test). split=None: at (13, 32)
# and (14, 32) the first splits do not fit LDS; at (11, 16), (12, 32), (13, 8) and (14, 32) further
# layers move out for one more wave per CU; at (10, 8) neither loop of the rule acts.
AUTO_CHOICE = {
    (10, 8, None): (1, 18192, 18432), (10, 8, 4): (4, 2992, 33792),
    (11, 16, None): (3, 20032, 125952), (11, 16, 2): (2, 37424, 108544),
    (12, 32, None): (6, 18144, 564736), (12, 32, 3): (3, 78976, 503808),
    (13, 8, None): (5, 13104, 278016), (13, 8, 1): (1, 143632, 147456),
    (13, 32, None): (3, 156800, 1007616), (13, 32, 4): (4, 87200, 1077248),
    (14, 32, None): (7, 51456, 2276352), (14, 32, 5): (5, 103616, 2224128),
}


@pytest.mark.gpu
def test_tiered_auto_choice_pinned():
    """What split=None chooses, and the layout sizes at it and at one explicit split: creation
    only, nothing is decoded. grid is left out (it follows the CU count and BCHK_POLAR_WORKSPACE_MB)."""
    for (n, L, ask), want in AUTO_CHOICE.items():
        d = tiered(arikan_spec(n, 1 << (n - 1)), L, ask)
        st = d.state_info()
        d.close()
        assert (st["split"], st["lds_bytes"], st["workspace_bytes"]) == want, (n, L, ask)


LONG = sorted(glob.glob(os.path.join(GOLD, "long_ref_*.txt.gz")))


def test_long_fixtures_are_present():
    assert len(LONG) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("path", LONG, ids=[os.path.basename(p)[9:-7] for p in LONG])
def test_gpu_tiered_matches_recorded_reference(path):
    """Past the C oracle (U > 4096): the recorded lists of the compiled vendored library."""
    fx = load_fixture(path)
    llr = fx.llr
    for L in fx.list_sizes:
        cnt, info, cw, met = tiered(fx.spec, L).decode(llr)
        for b, (c, winfo, wcw, wmet) in enumerate(fx.decoded(L)):
            assert cnt[b] == c, f"row {b}"
            np.testing.assert_array_equal(info[b, :c], winfo, err_msg=f"info, row {b}")
            np.testing.assert_array_equal(cw[b, :c], wcw, err_msg=f"codewords, row {b}")
            np.testing.assert_array_equal(met[b, :c].view(np.uint32), wmet, err_msg=f"metrics, row {b}")


@pytest.mark.gpu
def test_gpu_tiered_sweep():
    import torch
    from test_polar_sim import Batch, _sync, _zeros
    spec = arikan_spec(8, 128, dyn=6, seed=8)
    a = tiered(spec, 4).sweep_device(1.0, 1.0, 2, 2000, 20, seed=3)
    b = gpu_decoder(spec, 4).sweep_device(1.0, 1.0, 2, 2000, 20, seed=3)
    assert a[0] == b[0] and a[2] == b[2]
    # a code only the tiered state takes: one point against its three steps done by hand
    d = tiered(arikan_spec(12, 2048), 32)
    (pt,), _, words = d.sweep_device(1.5, 1.0, 1, 64, 1 << 40, seed=5)
    assert words == 64
    out8 = _zeros((8,), torch.int64)
    _sync()
    Batch(d, 1.5, 64, 5).count_device(0, 64, out8)
    assert pt[1] == [int(v) for v in out8.cpu().numpy()]
    assert pt[1][0] == 64


@pytest.mark.gpu
def test_gpu_tiered_workspace_and_caller_stream():
    import torch
    spec, o, info, llr = workload(9, 256, 10, (), 2.0, 200, seed=31)
    L, split, U = 8, 4, 512
    d = tiered(spec, L, split)
    st = d.state_info()
    # S_1..S_split of L arrays (floats) and the packed C_0..C_split (U, U, U/2, .. bits) of L arrays
    per_wg = 4 * L * (U - (U >> split)) + L * (U + sum(U >> (lam - 1) for lam in range(1, split + 1))) // 8
    assert st["workspace_bytes"] >= per_wg and st["grid"] >= 1
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
