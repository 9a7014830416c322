"""A plain SC-list decoder of Arikan polar codes in numpy float32, written from the decoding rule
and not from the library's data structures: the reference of the oracle where the oracle restates
the library's own scheme (dynamic frozen values kept as a 64-bit mask per path with a correction
word per symbol).

Here a path is its whole vector u of encoder inputs decided so far. A frozen symbol's value is the
XOR of its constraint's listed terms read from u; the "known" operands of the g steps are u's
segments encoded again, no partial-sum arrays are kept. What is shared with the library on purpose,
since lists are compared bit for bit: min-sum f and g in float32 (SoftProcessing.cpp:39-80), the
candidate order std::greater<pair<float, index>> with index 2 path + bit (MixedKernelListDecoder
.cpp:125), the path metric (a decision against the LLR's sign costs |LLR|), and which free path
index a clone takes (misc.h:203-226: a stack holding 0 .. L-1, L-1 on top; killed paths' indices
pushed in index order before the clones pop).

Only tests/ import this.
"""
import numpy as np

from polar_lib import spec_constraints

F32 = np.float32


def encode(u):
    """x = u G of the length-2^n Arikan transform: pairs (a, b) -> (a ^ b, b) at strides 1, 2, 4 .."""
    x = np.array(u, np.uint8)
    s = 1
    while s < len(x):
        v = x.reshape(-1, 2, s)
        v[:, 0, :] ^= v[:, 1, :]
        s *= 2
    return x


def f_step(a, b):
    m = np.minimum(np.abs(a), np.abs(b))
    return np.where(np.signbit(a) != np.signbit(b), -m, m).astype(F32)


def g_step(a, b, known):
    return np.where(known != 0, b - a, b + a).astype(F32)


class Path:
    def __init__(self, y, n):
        self.u = np.zeros(len(y), np.uint8)
        self.R = F32(0.0)
        self.S = [y] + [None] * n  # S[j]: the LLRs of the length 2^(n-j) sub-code in progress

    def clone(self):
        p = Path.__new__(Path)
        p.u, p.R, p.S = self.u.copy(), self.R, list(self.S)  # the LLR arrays are never written in place
        return p

    def leaf_llr(self, phi, n):
        """The LLR of u[phi] given u[0, phi): the levels below the lowest set bit of phi are
        computed again, the first of them by g with the sub-code word decided there."""
        m = 0 if phi == 0 else n - 1 - ((phi & -phi).bit_length() - 1)
        for j in range(m, n):
            h = 1 << (n - j - 1)
            a, b = self.S[j][:h], self.S[j][h:]
            if (phi >> (n - j - 1)) & 1:
                self.S[j + 1] = g_step(a, b, encode(self.u[phi - h:phi]))
            else:
                self.S[j + 1] = f_step(a, b)
        return self.S[n][0]


# Unfrozen phases decoded since the last STATS.update(...): all of them; those with more than L
# candidates, where cand[:L] cuts; of these the phases in which a path is killed, another goes on
# with one bit only and a third is cloned, all at once; and those where the cut falls between the
# two candidates of one path -- the last candidate kept and the first one dropped are one path's.
STATS = {"unfrozen": 0, "cut": 0, "three": 0, "split_pair": 0}


def decode(spec, llr, L):
    """llr [U] f32 -> (count, info [count][K], codewords [count][U], metrics f32 [count]), the
    list in the library's order. Arikan layers only, nothing shortened or punctured."""
    head = spec.split()
    U, K, n = int(head[0]), int(head[1]), int(head[3])
    assert U == 1 << n and head[4:6] == ["0", "0"] and head[6:6 + n] == ["A"] * n
    terms = {c[-1]: c[:-1] for c in spec_constraints(spec)}
    free = list(range(L))
    paths = {free.pop(): Path(np.ascontiguousarray(llr, F32), n)}
    for phi in range(U):
        v = {l: p.leaf_llr(phi, n) for l, p in paths.items()}
        if phi in terms:
            for l, p in paths.items():
                bit = 0
                for t in terms[phi]:
                    bit ^= int(p.u[t])
                if (bit != 0) != bool(v[l] < 0):
                    p.R = F32(p.R - np.abs(v[l]))
                p.u[phi] = bit
            continue
        cand = []
        for l in sorted(paths):
            hard = int(v[l] < 0)
            cand.append((float(paths[l].R), 2 * l + hard))
            cand.append((float(F32(paths[l].R - np.abs(v[l]))), 2 * l + (hard ^ 1)))
        cand.sort(reverse=True)
        keep = {}
        for r, i in cand[:L]:
            keep.setdefault(i >> 1, []).append(i & 1)
        STATS["unfrozen"] += 1
        if len(cand) > L:
            STATS["cut"] += 1
            bits = [len(b) for b in keep.values()]
            STATS["three"] += len(keep) < len(paths) and 1 in bits and 2 in bits
            STATS["split_pair"] += cand[L - 1][1] >> 1 == cand[L][1] >> 1
        for l in sorted(paths):
            if l not in keep:
                del paths[l]
                free.append(l)
        for l in sorted(keep):
            p = paths[l]
            if len(keep[l]) == 1:
                p.u[phi] = keep[l][0]
                continue
            q = p.clone()
            hard = int(v[l] < 0)
            p.u[phi], q.u[phi] = hard, hard ^ 1
            q.R = F32(p.R - np.abs(v[l]))
            paths[free.pop()] = q
    order = sorted(((float(p.R), l) for l, p in paths.items()), reverse=True)
    unfrozen = [i for i in range(U) if i not in terms]
    assert len(unfrozen) == K
    return (len(order), np.array([paths[l].u[unfrozen] for _, l in order], np.uint8),
            np.array([encode(paths[l].u) for _, l in order], np.uint8),
            np.array([paths[l].R for _, l in order], F32))
