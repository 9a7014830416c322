"""The n <= 63 first pass's claim logic, pinned to the C oracle at the smallest shapes where
each piece of it can go wrong (GPU box). BCH(63,30,13), J = 15, through the bench's call
(bchk_decode_count_device: words, l0 bits, six fused counters) and through the stats call
(bchk_decode_device: the three per-word counters).

The first pass (kaneko_search_kernel, AN = false) takes the words the ring kernel queued:
wave g takes item g without an atomic; the items from `stride` (the resident waves) upward
are claimed one at a time from eight sub-queues (sub-queue x: stride + x + 8 k), a wave's own
XCD's first, then the others'. `stride` is read from the context (first_pass_waves), never
assumed. (Claims of several entries at a time in the back of the queue, and a fetch of the
next row ahead, were measured and rejected: DESIGN 5.11. The cases below are the ones set
for them too, with a claim size of 1.)

Words: random codewords (info(x) g(x)) + AWGN from numpy's default_rng, so the test needs no
GPU to know what it feeds. The queue length is the number of words the oracle does not
resolve at test pattern 0 or 1 (decodes > 2); the ring kernel may send a few more on (prefix
ties), so every case asserts on the measured length (path_counts) as well.

Counts of the pools below (numpy default_rng, oracle, recorded on the CPU):
    6 dB seed 61, 4 096 words: 3 not resolved at pattern 0 or 1
    5 dB seed 51, 961 words: 17;  65 473 words: 1 799 (62 of them past the first pass's 8 chunks)
    4 dB seed 41, 65 535 words: 10 865 (1 269 past the 8 chunks)
With the default grid (5 120 waves on a 256-CU device) 2^16 words at 5 dB queue fewer words
than there are waves. The cases that need claims therefore run with one first-pass workgroup
per CU (BCHK_FIRST_PER_CU=1, stride = 4 x CUs).
"""
import os

import numpy as np
import pytest

from bchk_pkg import load
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

M, T, J = 6, 6, 15
POOLS = {6.0: (61, 4096), 5.0: (51, 65473), 4.0: (41, 65535)}
RECORDED = {(6.0, 4096): 3, (5.0, 961): 17, (5.0, 65473): 1799, (4.0, 65535): 10865}
_pool = {}
_dec = {}


def pool(snr):
    """(tx, y, oracle result) of the SNR's word pool, built and decoded once."""
    if snr not in _pool:
        seed, n_words = POOLS[snr]
        o = Oracle(M, T)
        rng = np.random.default_rng(seed)
        info = rng.integers(0, 2, (n_words, o.k), dtype=np.uint8)
        G = np.zeros((o.k, o.n), np.uint8)
        for i in range(o.k):
            G[i, i:i + len(o.g)] = o.g
        tx = ((info.astype(np.int32) @ G.astype(np.int32)) & 1).astype(np.uint8)
        y = (2.0 * tx - 1.0) + o.sigma(snr) * rng.standard_normal((n_words, o.n))
        _pool[snr] = (tx, y, o.kaneko_batch(y, J=J))
    return _pool[snr]


def decoder(per_cu=None, heavy_first=None):
    """A context with the given environment knobs (read at bchk_create), kept per setting."""
    key = (per_cu, heavy_first)
    if key not in _dec:
        knobs = {"BCHK_FIRST_PER_CU": per_cu, "BCHK_HEAVY_FIRST": heavy_first}
        old = {k: os.environ.get(k) for k in knobs}
        try:
            for k, v in knobs.items():
                if v is not None:
                    os.environ[k] = str(v)
            _dec[key] = load().KanekoKernelProcessor(M, T, J=J)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
    return _dec[key]


def counters_from(tx, res, dec, cmp, sums):
    err = (res != tx).sum(axis=1)
    return np.array([int((err > 0).sum()), int(err.sum()), int(dec.sum()), int(cmp.sum()), int(sums.sum()),
                     len(tx)], np.int64)


def check(d, snr, B, table=True):
    """Both calls over the pool's first B words against the oracle; returns the queue length."""
    import torch
    F = load()
    tx, y, (r2, l2, s2, a2) = pool(snr)
    tx, y, r2, l2, s2, acc = tx[:B], y[:B], r2[:B], l2[:B], s2[:B], a2[:B].astype(bool)
    d.set_syndrome_table(table)
    dy, dtx = torch.from_numpy(y).cuda(), torch.from_numpy(tx).cuda()
    dres = torch.zeros((B, d.n), dtype=torch.uint8, device="cuda")
    dl0 = torch.zeros(B, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(6, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d.decode_count_device(dy.data_ptr(), dtx.data_ptr(), B, dres.data_ptr(), dl0.data_ptr(), 0, cnt.data_ptr(),
                          d.stream)
    d.sync()
    queued = d.path_counts()[0]
    res, l0, cnt = dres.cpu().numpy(), dl0.cpu().numpy(), cnt.cpu().numpy()
    ores = np.where(acc[:, None], r2, 0)  # never accepted: the caller's zeros
    np.testing.assert_array_equal(res, ores)
    np.testing.assert_array_equal(l0[acc].view(np.uint64), l2[acc].view(np.uint64))
    want = counters_from(tx, ores, s2[:, 0], s2[:, 1], s2[:, 2])
    print(f"\n{snr} dB B={B} table={table}: queued {queued} (oracle {int((s2[:, 0] > 2).sum())}), "
          f"waves {d.first_pass_waves()}, counters {cnt.tolist()}")
    assert cnt[5] == B  # every word once
    assert cnt[2] == int(s2[:, 0].sum())  # no word decoded twice, none skipped
    np.testing.assert_array_equal(cnt, want)
    # the per-word counters: the same words with a stats record
    dres.zero_()
    dst = torch.zeros((B, F.STATS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d.decode_device(dy.data_ptr(), B, dres.data_ptr(), dl0.data_ptr(), dst.data_ptr(), d.stream)
    d.sync()
    st = dst.cpu().numpy().view(F.STATS_DTYPE).reshape(B)
    np.testing.assert_array_equal(dres.cpu().numpy(), ores)
    np.testing.assert_array_equal(dl0.cpu().numpy()[acc].view(np.uint64), l2[acc].view(np.uint64))
    np.testing.assert_array_equal(st["decodes"], s2[:, 0])
    np.testing.assert_array_equal(st["comparisons"], s2[:, 1])
    np.testing.assert_array_equal(st["sums"], s2[:, 2])
    np.testing.assert_array_equal((st["flags"] & F.F_ACCEPTED) != 0, acc)
    return queued


def oracle_queue(snr, B):
    return int((pool(snr)[2][2][:B, 0] > 2).sum())


@pytest.mark.parametrize("snr,B", [(6.0, 4096), (5.0, 961)])
def test_fewer_queued_words_than_waves(snr, B):
    # only the waves' own items run (no claim at all); 961 = 64 * 15 + 1 words leave fewer
    # than 64 queued
    d = decoder()
    assert oracle_queue(snr, B) == RECORDED[(snr, B)]
    waves = d.first_pass_waves()
    queued = check(d, snr, B)
    assert 0 < queued < waves
    if B == 961:
        assert queued < 64


@pytest.mark.parametrize("table", [True, False])
def test_queue_a_little_longer_than_the_waves(table):
    # static items, then at most one claim per sub-queue (some sub-queues empty), then the
    # exhaustion of all eight: the queue length is steered into (stride, stride + 8) by the
    # batch size
    d = decoder(per_cu=1)
    d.set_syndrome_table(table)
    waves, batch = d.first_pass_waves(), 1
    dec = pool(5.0)[2][2][:, 0]
    cum = np.cumsum(dec > 2)
    assert cum[-1] > waves + 8 * batch, "the 5 dB pool is too small for this device's grid"
    target = waves + 4 * batch
    for _ in range(3):  # the ring kernel may queue a few more than the oracle's count
        B = int(np.searchsorted(cum, target)) + 1
        queued = check(d, 5.0, B, table)
        if waves < queued < waves + 8 * batch:
            break
        target -= queued - (waves + 4 * batch)
    assert waves < queued < waves + 8 * batch


@pytest.mark.parametrize("heavy_first", [None, 0])
@pytest.mark.parametrize("snr,B", [(4.0, 65535), (5.0, 65473)])
def test_claims_across_the_front(snr, B, heavy_first):
    # 64 k + 63 and 64 k + 1 words; one workgroup per CU, so that the claims run through the
    # front of the queue into its back (filled from the end of the buffer), steal from the
    # other XCDs' sub-queues and meet the cw < count guard. Without the heavy-first order
    # there is no front.
    d = decoder(per_cu=1, heavy_first=heavy_first)
    assert oracle_queue(snr, B) == RECORDED[(snr, B)]
    waves = d.first_pass_waves()
    queued = check(d, snr, B)
    assert queued > waves + 8
