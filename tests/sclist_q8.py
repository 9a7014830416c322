"""The fixed-point SC-list decoder of Arikan polar codes, restated: the scheme of sclist_plain.py
(a path is its vector u; frozen values read from u; the known operands of the g steps are u's
segments encoded again) with the int8 arithmetic contract of include/bchk.h and DESIGN 5.18 in
numpy integers:

  load    -128 reads as -127; a punctured symbol is 0, a shortened one +127
  f       sgn(a) sgn(b) min(|a|, |b|)                 (0 if either operand is 0)
  g       clamp(u ? b - a : b + a, -127, +127)
  metric  an integer R; a decision against the hard decision v < 0 costs |v|

The list order is sclist_plain's: candidates by (R, 2 path + bit) descending, killed paths'
indices pushed in index order before the clones pop, the final list by (R, path) descending. The
length-U LLR vector is built here from the specification's shortened and punctured lists, so
shortened codes are covered; codewords are returned over the transmitted symbols.

Only tests/ import this.
"""
import numpy as np

from polar_lib import spec_constraints
from sclist_plain import encode

QMAX = 127
I32 = np.int32


def load_llrs(spec, q):
    """The U LLRs of the unshortened code from the row q [N] (int8): (llr int32 [U], transmitted
    positions)."""
    tok = spec.split()
    N, layers, nsh, npu = int(tok[0]), int(tok[3]), int(tok[4]), int(tok[5])
    U = N + nsh + npu
    marked = [int(v) for v in tok[6 + layers:6 + layers + nsh + npu]]
    short, punct = set(marked[:nsh]), set(marked[nsh:])
    sent = [i for i in range(U) if i not in short and i not in punct]
    y = np.zeros(U, I32)
    y[sent] = np.maximum(np.asarray(q, np.int8).astype(I32), -QMAX)
    y[sorted(short)] = QMAX
    return y, sent


def f_step(a, b):
    m = np.minimum(np.abs(a), np.abs(b))
    return np.where((a < 0) != (b < 0), -m, m).astype(I32)


# g-step outputs formed, and how many of them saturated; decode() adds "split_pair", the unfrozen
# phases whose cut falls between the two candidates of one path (sclist_plain.STATS)
STATS = {"g": 0, "clamped": 0}


def g_step(a, b, known):
    r = np.where(known != 0, b - a, b + a)
    STATS["g"] += r.size
    STATS["clamped"] += int((np.abs(r) > QMAX).sum())
    return np.clip(r, -QMAX, QMAX).astype(I32)


class Path:
    def __init__(self, y, n):
        self.u = np.zeros(len(y), np.uint8)
        self.R = 0
        self.S = [y] + [None] * n  # S[j]: the LLRs of the length 2^(n-j) sub-code in progress

    def clone(self):
        p = Path.__new__(Path)
        p.u, p.R, p.S = self.u.copy(), self.R, list(self.S)  # the LLR arrays are never written in place
        return p

    def leaf_llr(self, phi, n):
        m = 0 if phi == 0 else n - 1 - ((phi & -phi).bit_length() - 1)
        for j in range(m, n):
            h = 1 << (n - j - 1)
            a, b = self.S[j][:h], self.S[j][h:]
            if (phi >> (n - j - 1)) & 1:
                self.S[j + 1] = g_step(a, b, encode(self.u[phi - h:phi]))
            else:
                self.S[j + 1] = f_step(a, b)
        return int(self.S[n][0])


def decode(spec, q, L):
    """q [N] int8 -> (count, info [count][K], codewords [count][N], metrics int64 [count]), the
    list in the decoder's order. Arikan layers only."""
    head = spec.split()
    K, n = int(head[1]), int(head[3])
    assert head[6:6 + n] == ["A"] * n
    y, sent = load_llrs(spec, q)
    U = len(y)
    assert U == 1 << n
    terms = {c[-1]: c[:-1] for c in spec_constraints(spec)}
    free = list(range(L))
    paths = {free.pop(): Path(y, n)}
    for phi in range(U):
        v = {l: p.leaf_llr(phi, n) for l, p in paths.items()}
        if phi in terms:
            for l, p in paths.items():
                bit = 0
                for t in terms[phi]:
                    bit ^= int(p.u[t])
                if (bit != 0) != (v[l] < 0):
                    p.R -= abs(v[l])
                p.u[phi] = bit
            continue
        cand = []
        for l in sorted(paths):
            hard = int(v[l] < 0)
            cand.append((paths[l].R, 2 * l + hard))
            cand.append((paths[l].R - abs(v[l]), 2 * l + (hard ^ 1)))
        cand.sort(reverse=True)
        if len(cand) > L:  # as sclist_plain.STATS counts it: the cut falls between one path's two candidates
            STATS["split_pair"] = STATS.get("split_pair", 0) + (cand[L - 1][1] >> 1 == cand[L][1] >> 1)
        keep = {}
        for r, i in cand[:L]:
            keep.setdefault(i >> 1, []).append(i & 1)
        for l in sorted(paths):
            if l not in keep:
                del paths[l]
                free.append(l)
        for l in sorted(keep):
            p = paths[l]
            if len(keep[l]) == 1:
                p.u[phi] = keep[l][0]
                continue
            c = p.clone()
            hard = int(v[l] < 0)
            p.u[phi], c.u[phi] = hard, hard ^ 1
            c.R = p.R - abs(v[l])
            paths[free.pop()] = c
    order = sorted(((p.R, l) for l, p in paths.items()), reverse=True)
    unfrozen = [i for i in range(U) if i not in terms]
    assert len(unfrozen) == K
    return (len(order), np.array([paths[l].u[unfrozen] for _, l in order], np.uint8).reshape(len(order), K),
            np.array([encode(paths[l].u)[sent] for _, l in order], np.uint8),
            np.array([paths[l].R for _, l in order], np.int64))
