"""Genie-aided SC restated in numpy / float32: single-path successive cancellation over mixed
kernels with the TRUE earlier symbols fed back, the checker of csrc/polar_genie.hip.

Written from DESIGN.md §5.5 and oracle/polar_oracle.c (which it only reads): LoadLLRs, then per
phase IterativelyCalcS -- f/g on Arikan layers as recursive_sc of tests/test_polar_oracle.py
forms them, matrix layers through the oracle's exported plr_minsum_llr (ctypes, oracle/build/
libpolar_oracle.so) on the offset-flipped LLRs -- and IterativelyUpdateC with the true u_phi.
Also the encoder's input u from the information bits, and the per-symbol statistics of
include/bchk.h (bchk_polar_genie_device).

Only tests/ import this.
"""
import ctypes as C
import os

import numpy as np

from polar_lib import lib as plib


class _PK(C.Structure):  # plr_kernel (oracle/polar_oracle.c)
    _fields_ = [("size", C.c_int), ("arikan", C.c_int), ("K", C.c_uint8 * 4096), ("Kinv", C.c_uint8 * 4096)]


def _plr_kernel(K):
    k = _PK()
    k.size, k.arikan = len(K), 0
    for i, v in enumerate(np.asarray(K, np.uint8).ravel()):
        k.K[i] = int(v)
    return k


def _minsum():
    L = plib()
    L.plr_minsum_llr.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.plr_minsum_llr.restype = C.c_float
    return L.plr_minsum_llr


class GenieCode:
    """One code from its specification text (the reference's format, as bchk_polar_create_kdir
    reads it): layers, shortened / punctured symbols, freezing constraints."""

    def __init__(self, spec, kernel_dir=None):
        tok = spec.split()
        N, K, _, nl, nsh, npu = (int(t) for t in tok[:6])
        pos = 6
        self.kernels = []  # None = Arikan, else the l x l matrix
        for name in tok[pos:pos + nl]:
            if name in ("A", "a"):
                self.kernels.append(None)
            else:
                path = name[1:]
                if kernel_dir and not os.path.isabs(path):
                    path = os.path.join(kernel_dir, path)
                t = open(path).read().split()
                l = int(t[0])
                self.kernels.append(np.array(t[1:1 + l * l], np.uint8).reshape(l, l))
        pos += nl
        self.sizes = [2 if k is None else len(k) for k in self.kernels]
        self.U = int(np.prod(self.sizes))
        self.N, self.K, self.nl = N, K, nl
        assert N + nsh + npu == self.U
        self.symtype = np.zeros(self.U, np.uint8)
        for i in range(nsh + npu):
            self.symtype[int(tok[pos + i])] = 1 if i < nsh else 2
        pos += nsh + npu
        self.constraint = [None] * self.U  # terms before the frozen symbol
        for _ in range(self.U - K):
            w = int(tok[pos])
            terms = [int(t) for t in tok[pos + 1:pos + 1 + w]]
            pos += 1 + w
            self.constraint[terms[-1]] = terms[:-1]
        self.frozen = np.array([c is not None for c in self.constraint])
        self.outer = [self.U]
        for l in self.sizes:
            self.outer.append(self.outer[-1] // l)
        self._pk = [None if k is None else _plr_kernel(k) for k in self.kernels]
        self._llr = _minsum()

    def build_u(self, info):
        """The encoder's input: information bits at the unfrozen symbols, a frozen symbol the XOR
        of its constraint's earlier terms (0 for a static one), in symbol order."""
        u = np.zeros(self.U, np.uint8)
        k = 0
        for i in range(self.U):
            if self.constraint[i] is None:
                u[i] = info[k] & 1
                k += 1
            else:
                for t in self.constraint[i]:
                    u[i] ^= u[t]
        return u

    def load_llrs(self, llr):
        """LoadLLRs: 100000 at shortened symbols, 0 at punctured ones."""
        chan = np.zeros(self.U, np.float32)
        chan[self.symtype == 0] = np.asarray(llr, np.float32)
        chan[self.symtype == 1] = np.float32(100000.0)
        return chan

    def sc_llrs(self, llr, u):
        """LLR_phi for phi = 0..U-1 of one word, u_0..u_{phi-1} fed back true (float32 [U])."""
        nl, sizes, outer = self.nl, self.sizes, self.outer
        S = [self.load_llrs(llr)] + [np.zeros(outer[lam], np.float32) for lam in range(1, nl + 1)]
        Cs = [np.zeros(self.U, np.uint8)] + [np.zeros(outer[lam] * sizes[lam - 1], np.uint8) for lam in range(1, nl + 1)]
        O = [None if self.kernels[j] is None else np.zeros(sizes[j] * outer[j + 1], np.uint8) for j in range(nl)]
        out = np.zeros(self.U, np.float32)
        for phi in range(self.U):
            m, pq = nl - 1, phi
            while m > 0 and pq % sizes[m] == 0:
                pq //= sizes[m]
                m -= 1
            for j in range(m, nl):
                loc = pq % sizes[j] if j == m else 0
                d, l = outer[j + 1], sizes[j]
                src, known = S[j], Cs[j + 1]
                if self.kernels[j] is None:
                    a, b = src[:d], src[d:2 * d]
                    if loc == 0:
                        mn = np.minimum(np.abs(a), np.abs(b))
                        S[j + 1] = np.where(np.signbit(a) != np.signbit(b), -mn, mn).astype(np.float32)
                    else:
                        S[j + 1] = np.where(known[:d] != 0, b - a, b + a).astype(np.float32)
                    continue
                Kj, off = self.kernels[j], O[j]
                if loc == 0:
                    off[:] = 0
                else:
                    kn = known[(loc - 1) * d:loc * d]
                    for i in range(l):
                        if Kj[loc - 1, i]:
                            off[i * d:(i + 1) * d] ^= kn
                y = np.where(off != 0, -src[:l * d], src[:l * d]).astype(np.float32).reshape(l, d)
                dst = np.zeros(d, np.float32)
                for s in range(d):
                    col = np.ascontiguousarray(y[:, s])
                    dst[s] = self._llr(C.byref(self._pk[j]), int(loc), col.ctypes.data_as(C.c_void_p))
                S[j + 1] = dst
            out[phi] = S[nl][0]
            Cs[nl][phi % sizes[nl - 1]] = u[phi]
            lam, stride, ph = nl, 1, phi
            while lam > 0 and (ph + 1) % sizes[lam - 1] == 0:
                l = sizes[lam - 1]
                psi = ph // l
                nxt = stride * l
                phi0 = (psi % sizes[lam - 2]) * nxt if lam > 1 else 0
                x = Cs[lam][:nxt].reshape(l, stride)
                if self.kernels[lam - 1] is None:
                    yv = np.concatenate([x[0] ^ x[1], x[1]])
                else:
                    Km = self.kernels[lam - 1]
                    yv = ((x.T.astype(np.int64) @ Km.astype(np.int64)) & 1).astype(np.uint8).T.reshape(-1)
                Cs[lam - 1][phi0:phi0 + nxt] = yv
                stride, ph, lam = nxt, psi, lam - 1
        return out


def decisions_wrong(dec_llr, u):
    """(LLR < 0 ? 1 : 0) != u, the decoder's decision rule, per symbol."""
    return (np.asarray(dec_llr) < 0) != (np.asarray(u) != 0)


def soft_q(dec_llr, u):
    """The quantised soft value of include/bchk.h: s = u ? -LLR : LLR clamped to [-32768, 32768],
    times 65536 (exact in float32), rounded to nearest even, as int64."""
    v = np.asarray(dec_llr, np.float32)
    s = np.where(np.asarray(u) != 0, -v, v).astype(np.float32)
    c = np.clip(s, np.float32(-32768.0), np.float32(32768.0)).astype(np.float32)
    return np.rint(c * np.float32(65536.0)).astype(np.int64)


def column_sums(dec_llr, u):
    """(err [U] uint64, soft [U] int64) of rows dec_llr [B][U], u [B][U]."""
    return decisions_wrong(dec_llr, u).sum(axis=0).astype(np.uint64), soft_q(dec_llr, u).sum(axis=0)


def first_wrong_unfrozen(code, dec_llr, u):
    """Index among the unfrozen symbols of the first one the decision rule gets wrong, or None."""
    bad = np.flatnonzero(decisions_wrong(dec_llr, u) & ~code.frozen)
    return None if len(bad) == 0 else int(np.count_nonzero(~code.frozen[:bad[0]]))


def frozen_penalty(code, dec_llr, u):
    """The SC path metric of a correctly decoded word: the float32 sum, in symbol order from 0, of
    -|LLR_phi| over the frozen phi whose LLR contradicts u_phi."""
    r = np.float32(0.0)
    for phi in np.flatnonzero(decisions_wrong(dec_llr, u) & code.frozen):
        r = np.float32(r - np.abs(np.float32(dec_llr[phi])))
    return r


def rank_frozen(err, soft, K):
    """design_genie's rule: i is better than j when err_i < err_j, then soft_i > soft_j, then i > j;
    the K best carry information. Returns the frozen symbols, ascending."""
    U = len(err)
    order = sorted(range(U), key=lambda i: (int(err[i]), -int(soft[i]), -i))
    return sorted(order[K:])
