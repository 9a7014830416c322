"""CPU truth for the BEC polarisation tests (test_kernel_bec.py, test_polar_design.py): which
phases of a polar kernel an erasure pattern leaves uncorrectable, as a vectorised XOR basis in
numpy. Written independently of csrc/kernel_bec.hip: the basis here is keyed by the highest set
bit and holds one array per bit position over all patterns.

Only tests/ import this.
"""
from math import comb

import numpy as np


def row_masks(K):
    return [sum(int(v) << c for c, v in enumerate(row)) for row in np.asarray(K)]


def np_masks(K, patterns):
    """patterns: uint64 (bit j = column j erased) -> uint64 masks, bit i = phase i is
    uncorrectable: row_i restricted to the kept columns lies in the span of the rows below."""
    l = len(K)
    rows = row_masks(K)
    pat = np.ascontiguousarray(patterns, np.uint64)
    keep = ~pat
    basis = np.zeros((l, pat.size), np.uint64)
    unc = np.zeros(pat.size, np.uint64)
    one = np.uint64(1)
    for i in range(l - 1, -1, -1):
        v = np.uint64(rows[i]) & keep
        inserted = np.zeros(pat.size, bool)
        for bit in range(l - 1, -1, -1):
            has = ((v >> np.uint64(bit)) & one).astype(bool) & ~inserted
            if not has.any():
                continue
            filled = basis[bit] != 0
            red = has & filled
            v = np.where(red, v ^ basis[bit], v)
            ins = has & ~filled
            basis[bit] = np.where(ins, v, basis[bit])
            inserted |= ins
        unc |= (~inserted).astype(np.uint64) << np.uint64(i)
    return unc


def popcount(a):
    a = np.ascontiguousarray(a, np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def histogram(l, patterns, masks):
    """counts [l][l + 1] (Python-int exact in uint64): patterns of weight w with bit i set."""
    w = popcount(patterns)
    counts = np.zeros((l, l + 1), np.uint64)
    for i in range(l):
        hit = ((masks >> np.uint64(i)) & np.uint64(1)).astype(bool)
        counts[i] = np.bincount(w[hit], minlength=l + 1).astype(np.uint64)
    return counts


def patterns_of_weights(l, weights):
    """Every l-bit pattern whose weight is in `weights`, as uint64."""
    from itertools import combinations
    out = []
    for w in weights:
        if w == 0:
            out.append(np.zeros(1, np.uint64))
            continue
        idx = np.array(list(combinations(range(l), w)), np.uint64)
        out.append((np.uint64(1) << idx).sum(axis=1, dtype=np.uint64))
    return np.concatenate(out)


def brute_mask(K, erased):
    """The definition, one pattern: span membership by enumerating the combinations of the rows
    below (small kernels only)."""
    l = len(K)
    rows = [r & ~erased for r in row_masks(K)]
    unc = 0
    for i in range(l):
        below = rows[i + 1:]
        span = {0}
        for r in below:
            span |= {s ^ r for s in span}
        if rows[i] in span:
            unc |= 1 << i
    return unc


def erasure_polynomial(counts_row, l, p):
    """sum_w counts[w] p^w (1 - p)^(l - w) in exact rational arithmetic."""
    from fractions import Fraction
    p = Fraction(p)
    return sum(int(c) * p ** w * (1 - p) ** (l - w) for w, c in enumerate(counts_row))


def binomials(l):
    return [comb(l, w) for w in range(l + 1)]
