"""BEC polarisation behaviour of polar kernels on the GPU (csrc/kernel_bec.hip): per erasure
pattern the phases it leaves uncorrectable (bchk_kernel_bec_masks), the exact table by
enumeration (bchk_kernel_bec_behaviour) and the sampled one (bchk_kernel_bec_sample) -- the
table the reference's CBECCapacityEvaluator reads (out/external/CapacityEvaluator.cpp:100-140)
but nothing in the reference produces. The truth is the numpy XOR basis of bec_lib.py."""
import os
from math import comb

import numpy as np
import pytest

from bchk_pkg import load
from bec_lib import brute_mask, histogram, np_masks, patterns_of_weights, popcount

F2 = np.array([[1, 0], [1, 1]], np.uint8)
TERNARY = np.array([[1, 1, 1], [1, 0, 1], [0, 1, 1]], np.uint8)


def random_invertible(l, seed):
    rng = np.random.default_rng(seed)
    while True:
        K = rng.integers(0, 2, (l, l)).astype(np.uint8)
        if round(abs(np.linalg.det(K.astype(float)))) % 2 == 1:
            return K


def kernels():
    b = load()
    return {"arikan": F2, "ternary": TERNARY, "rand5": random_invertible(5, 7), "ebch16": b.kernel_ebch(4),
            "ebch32": b.kernel_ebch(5), "ebch64": b.kernel_ebch(6)}


def probe_patterns(l):
    if l <= 16:
        return np.arange(1 << l, dtype=np.uint64)
    rng = np.random.default_rng(l)
    full = np.uint64((1 << l) - 1)
    rnd = rng.integers(0, 1 << 63, 4096, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 4096, dtype=np.uint64)
    single = np.uint64(1) << np.arange(l, dtype=np.uint64)
    return np.concatenate([rnd & full, np.array([0, full], np.uint64), single, full ^ single])


_cache = {}


def truth(name):
    """(patterns, numpy masks) of the probe patterns of one kernel, computed once."""
    if name not in _cache:
        K = kernels()[name]
        pat = probe_patterns(len(K))
        _cache[name] = (pat, np_masks(K, pat))
    return _cache[name]


def small_table(name):
    K = kernels()[name]
    pat, m = truth(name)
    return histogram(len(K), pat, m)


def test_numpy_checker_matches_the_definition():
    for K in (F2, TERNARY, random_invertible(5, 7), random_invertible(6, 3)):
        pat = np.arange(1 << len(K), dtype=np.uint64)
        assert [int(v) for v in np_masks(K, pat)] == [brute_mask(K, int(e)) for e in pat]
    # the hand check: phase 0 -> (2, 1), phase 1 -> (0, 1) for weights 1 and 2
    pat = np.arange(4, dtype=np.uint64)
    assert histogram(2, pat, np_masks(F2, pat)).tolist() == [[0, 2, 1], [0, 0, 1]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["arikan", "ternary", "rand5", "ebch16", "ebch32", "ebch64"])
def test_masks_match_numpy(name):
    K = kernels()[name]
    pat, want = truth(name)
    got = load().kernel_bec_masks(K, pat)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_singular_kernel_rejected():
    b = load()
    for l in (2, 5, 32, 64):
        K = np.eye(l, dtype=np.uint8)
        K[l - 1] = K[0]
        with pytest.raises(b.BchkError, match="singular"):
            b.kernel_bec_masks(K, np.zeros(1, np.uint64))
        if l <= 32:
            with pytest.raises(b.BchkError, match="singular"):
                b.kernel_bec_behaviour(K)
        with pytest.raises(b.BchkError, match="singular"):
            b.kernel_bec_sample(K, 16)
    with pytest.raises(b.BchkError):
        b.kernel_bec_behaviour(b.kernel_ebch(6))  # exact enumeration stops at 32


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["arikan", "ternary", "rand5", "ebch16"])
def test_enumeration_small_kernels(name):
    K = kernels()[name]
    l = len(K)
    want = small_table(name)
    got = load().kernel_bec_behaviour(K)
    assert np.array_equal(got, want)
    if name == "arikan":
        assert got.tolist() == [[0, 2, 1], [0, 0, 1]]
    # a weight range leaves the other weights 0
    part = load().kernel_bec_behaviour(K, 1, l - 1)
    assert np.array_equal(part[:, 1:l], want[:, 1:l]) and not part[:, 0].any() and not part[:, l].any()


@pytest.mark.gpu
def test_enumeration_32_extreme_weights():
    K = kernels()["ebch32"]
    full = np.uint64((1 << 32) - 1)
    low = patterns_of_weights(32, range(6))  # 242 825 patterns
    got_lo = load().kernel_bec_behaviour(K, 0, 5)
    got_hi = load().kernel_bec_behaviour(K, 27, 32)
    assert np.array_equal(got_lo, histogram(32, low, np_masks(K, low)))
    assert np.array_equal(got_hi, histogram(32, full ^ low, np_masks(K, full ^ low)))


def kron_power_table(n):
    """The table of F^{(x) n} (np.kron) in closed form. kron puts the first factor in the most
    significant index bit: c = (x0 + x1, x1) with x0, x1 the transforms of the halves u0, u1 by
    F^{(x) (n - 1)}, and u0 is decoded first. So the most significant bit transforms the channel
    itself -- erasure probability z -> 2z - z^2 for bit 0, z -> z^2 for bit 1 -- and the lower
    bits follow in order. The erasure polynomial of phase i in p, expanded in
    p^w (1 - p)^(l - w): p^k = sum_j C(l - k, j) p^(k + j) (1 - p)^(l - k - j)."""
    l = 1 << n

    def mul(a, b):
        r = [0] * (len(a) + len(b) - 1)
        for i, u in enumerate(a):
            for j, v in enumerate(b):
                r[i + j] += u * v
        return r

    table = []
    for i in range(l):
        z = [0, 1]
        for bit in range(n - 1, -1, -1):
            sq = mul(z, z)
            z = sq if (i >> bit) & 1 else [2 * a - b for a, b in zip(z + [0] * (len(sq) - len(z)), sq)]
        z = z + [0] * (l + 1 - len(z))
        table.append([sum(z[k] * comb(l - k, w - k) for k in range(w + 1)) for w in range(l + 1)])
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ebch32", "arikan5"])
def test_enumeration_32_full(name):
    """All 2^32 patterns: every pattern leaves exactly |S| phases correctable (K is invertible),
    so column w sums to w C(32, w); for the Kronecker power the table equals the closed form
    exactly. Measured on the MI355X: see DESIGN.md (well under the 10 s cap, so both kernels
    keep their full-range check)."""
    K = kernels()["ebch32"] if name == "ebch32" else np.kron(np.kron(np.kron(np.kron(F2, F2), F2), F2), F2)
    got = load().kernel_bec_behaviour(K)
    sums = [int(sum(int(v) for v in got[:, w])) for w in range(33)]
    assert sums == [w * comb(32, w) for w in range(33)]
    if name == "arikan5":
        assert [[int(v) for v in row] for row in got] == kron_power_table(5)


def test_closed_form_matches_numpy_on_8():
    K = np.kron(np.kron(F2, F2), F2)
    pat = np.arange(256, dtype=np.uint64)
    assert histogram(8, pat, np_masks(K, pat)).tolist() == kron_power_table(3)


@pytest.mark.gpu
def test_sampling_16():
    b = load()
    K = kernels()["ebch16"]
    want = small_table("ebch16")
    unc, tried, exact = b.kernel_bec_sample(K, 1 << 16)
    assert exact.all() and np.array_equal(unc, want)
    assert [int(t) for t in tried] == [comb(16, w) for w in range(17)]

    os.environ["BCHK_BEC_RUN"] = "1"
    try:
        unc, tried, exact = b.kernel_bec_sample(K, 1 << 12, seed=5)
        os.environ["BCHK_BEC_RUN"] = "37"
        again = b.kernel_bec_sample(K, 1 << 12, seed=5)
    finally:
        del os.environ["BCHK_BEC_RUN"]
    default = b.kernel_bec_sample(K, 1 << 12, seed=5)
    for other in (again, default):  # the lane / launch shape does not matter
        assert all(np.array_equal(x, y) for x, y in zip((unc, tried, exact), other))
    assert not np.array_equal(unc, b.kernel_bec_sample(K, 1 << 12, seed=6)[0])
    assert exact.tolist() == [comb(16, w) <= 4096 for w in range(17)] and not exact.all()
    for w in range(17):
        if exact[w]:
            assert np.array_equal(unc[:, w], want[:, w]) and int(tried[w]) == comb(16, w)
            continue
        n = int(tried[w])
        assert n == 4096
        for i in range(16):
            f = int(want[i, w]) / comb(16, w)
            sigma = (f * (1 - f) / n) ** 0.5
            bound = 5 * sigma if sigma > 0 else 1 / n  # 5 binomial standard deviations
            assert abs(int(unc[i, w]) / n - f) <= bound, (i, w, int(unc[i, w]), f)


@pytest.mark.gpu
def test_sampling_64():
    b = load()
    K = kernels()["ebch64"]
    w_s = 20
    unc, tried, exact, pat = b.kernel_bec_sample(K, 1 << 12, seed=3, pattern_weight=w_s)
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    single = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for w, p in ((0, np.zeros(1, np.uint64)), (1, single), (63, full ^ single), (64, np.array([full]))):
        assert exact[w] and int(tried[w]) == len(p)
        assert np.array_equal(unc[:, w], histogram(64, p, np_masks(K, p))[:, w])
    assert not exact[w_s] and int(tried[w_s]) == 4096 and len(pat) == 4096
    assert (popcount(pat) == w_s).all()
    assert len(np.unique(pat)) > 4000  # draws, not one pattern repeated
    assert np.array_equal(unc[:, w_s], histogram(64, pat, np_masks(K, pat))[:, w_s])
    # an enumerated weight hands out its patterns too, in rank order
    _, tried2, exact2, pat2 = b.kernel_bec_sample(K, 1 << 12, seed=3, pattern_weight=2)
    assert exact2[2] and len(pat2) == comb(64, 2) == len(np.unique(pat2)) and (popcount(pat2) == 2).all()
    assert (pat2[1:] > pat2[:-1]).all()
