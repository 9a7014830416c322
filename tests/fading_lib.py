"""CPU reference of the fading models with a parameter of the polar channel front-end
(bchk_polar_generate_fading_device: block Rayleigh, correlated Rayleigh, Rician), beside
tests/philox_lib.py and tests/channel_lib.py, which it extends and leaves as they are.

Written from the text of include/bchk.h (BCHK_FADING_*) and csrc/bchk_philox.h, not from the
kernel. Common to the three: y = h x + sigma z with x, sigma and z those of channel_lib's Rayleigh
channel; only h differs.
  block, size S:    positions [b S, (b + 1) S) of word w share h = sqrt(-log u(w N + b S)), u the
                    uniform of channel_lib (tag 0xFAD1)
  correlated, rho:  elements 2 q and 2 q + 1 of a word share h_q = sqrt((a_q^2 + b_q^2) / 2); a, b
                    are g_0 = z_0, g_q = rho g_{q-1} + c z_q over the Box-Muller pairs of counter
                    (w low, w high, 0xC022, q): element 0 for a, element 1 for b. rho and
                    c = sqrt(1 - rho^2) are the doubles the host forms; the reference carries
                    everything else in philox_lib's number type above double
  Rician, K:        h = sqrt((v + s z1)^2 + (s z2)^2) over the pair of counter (w low, w high,
                    0x21CE, position), v = sqrt(K / (K + 1)) and s = sqrt(1 / (2 (K + 1))) the
                    doubles the host forms
The device runs the same recursion in doubles (the product c z_q rounded, then one fused
multiply-add); tests/test_polar_fading.py bounds the distance between the two.

Only tests/ import this.
"""
import math
from decimal import localcontext

import numpy as np

import channel_lib as CL
import philox_lib as P

TAG_CORRELATED, TAG_RICIAN = 0xC022, 0x21CE
assert len({TAG_CORRELATED, TAG_RICIAN, CL.TAG_UNIFORM, P.TAG_INFO, P.TAG_NOISE}) == 5
assert TAG_CORRELATED > 64 and TAG_RICIAN > 64  # word 2 of a BEC draw is a weight of at most 64

BLOCK, CORRELATED, RICIAN = 0, 1, 2
KINDS = {"rayleigh_block": BLOCK, "rayleigh_correlated": CORRELATED, "rician": RICIAN}


def _ld(use_ld):
    return P.HAVE_LD if use_ld is None else use_ld


def scalar(x, use_ld):
    """One double in the reference's number type."""
    return P.lift(np.float64(x), _ld(use_ld)).reshape(-1)[0]


def words_of(B, use_ld=None):
    """How many of B words get a reference (all of them on the longdouble path)."""
    return B if _ld(use_ld) else min(B, P.DEC_WORDS)


def sqrt_ref(a):
    a = np.asarray(a)
    if a.dtype != object:
        return np.sqrt(a)
    with localcontext() as ctx:
        ctx.prec = P.DEC_PREC + 10
        return np.array([v.sqrt() for v in a.ravel()], dtype=object).reshape(a.shape)


def word_pairs(tag, count, seed, word0, B, use_ld=None):
    """(z0, z1), each [B][count] in the reference's number type: the Box-Muller pair of counter
    (w low, w high, tag, i) for i < count of words [word0, word0 + B)."""
    words = np.arange(B, dtype=np.uint64) + np.uint64(word0)
    lo, hi = P._split64(words)
    idx = np.arange(count, dtype=np.uint64)
    r = P.philox4x32_10((lo[:, None], hi[:, None], tag, idx[None, :]), (seed & 0xFFFFFFFF, seed >> 32))
    v1, v2 = P.unit53_int(r[0], r[1]).ravel(), P.unit53_int(r[2], r[3]).ravel()
    if _ld(use_ld):
        z0, z1 = P.normal_from_units_ld(v1, v2)
    else:
        z = [P.normal_from_units_dec(a, b) for a, b in zip(v1.tolist(), v2.tolist())]
        z0 = np.array([p[0] for p in z], dtype=object)
        z1 = np.array([p[1] for p in z], dtype=object)
    return z0.reshape(B, count), z1.reshape(B, count)


# ---------------------------------------------------------------- block Rayleigh

def block_units(N, S, seed, word0, B):
    """v [B][N] (u = v 2^-53) of the factors: position i takes the unit of the first element of
    its block, flat element w N + (i // S) S."""
    first = (np.arange(N) // int(S)) * int(S)
    return CL.word_units(N, seed, word0, B)[:, first]


def block_fading(N, S, seed, word0, B, use_ld=None):
    return CL.fading_from_units(block_units(N, S, seed, word0, B), _ld(use_ld))


# ---------------------------------------------------------------- correlated Rayleigh

def rho_c(rho):
    """(rho, c) as the doubles of the contract: c = sqrt(1 - rho^2), every operation rounded."""
    rho = np.float64(rho)
    return rho, np.sqrt(np.float64(1.0) - rho * rho)


def ar1(z, rho, use_ld=None):
    """g_0 = z_0, g_q = rho g_{q-1} + c z_q along the last axis, in the number type of z."""
    r, c = rho_c(rho)
    r, c = scalar(r, use_ld), scalar(c, use_ld)
    g = np.empty_like(z)
    g[..., 0] = z[..., 0]
    for q in range(1, z.shape[-1]):
        g[..., q] = r * g[..., q - 1] + c * z[..., q]
    return g


def ar1_cholesky(n, rho, use_ld=None):
    """The lower Cholesky factor of the covariance rho^|i-j| (n x n) in closed form:
    L[i][0] = rho^i, L[i][j] = c rho^(i-j) for 1 <= j <= i; with c^2 = 1 - rho^2 exactly, L L^T
    is that matrix (row i times row j, i >= j, telescopes to rho^(i-j))."""
    r, c = rho_c(rho)
    r, c, one = scalar(r, use_ld), scalar(c, use_ld), scalar(1.0, use_ld)
    Lm = np.full((n, n), one * 0, dtype=np.longdouble if _ld(use_ld) else object)
    for i in range(n):
        for j in range(i + 1):
            Lm[i, j] = (one if j == 0 else c) * r ** (i - j)
    return Lm


def correlated_gauss(N, rho, seed, word0, B, use_ld=None):
    """(a, b, ta, tb), each [B][(N + 1) / 2]: the two correlated sequences and the terms the
    recursion adds (z_0, then c z_q) -- the tests' bound needs their size."""
    nq = (N + 1) // 2
    za, zb = word_pairs(TAG_CORRELATED, nq, seed, word0, B, use_ld)
    c = scalar(rho_c(rho)[1], use_ld)
    ta, tb = c * za, c * zb
    ta[:, 0], tb[:, 0] = za[:, 0], zb[:, 0]
    return ar1(za, rho, use_ld), ar1(zb, rho, use_ld), ta, tb


def symbol_fading(a, b):
    """h_q = sqrt((a_q^2 + b_q^2) / 2)."""
    return sqrt_ref((a * a + b * b) / 2)


def spread(hq, N):
    """[B][nq] per QAM symbol -> [B][N] per element (the last symbol of an odd N is half filled)."""
    return np.repeat(hq, 2, axis=1)[:, :N]


# ---------------------------------------------------------------- Rician

def rice_vs(K):
    """(v, s) as the doubles the host forms. Omega = 2 s^2 + v^2 = 1 and K = v^2 / (2 s^2)."""
    K = np.float64(K)
    one = np.float64(1.0)
    return np.sqrt(K / (K + one)), np.sqrt(one / (np.float64(2.0) * (K + one)))


def rician_parts(N, K, seed, word0, B, use_ld=None):
    """(re, im, t1), each [B][N]: re = v + s z1, im = s z2, t1 = s z1."""
    z1, z2 = word_pairs(TAG_RICIAN, N, seed, word0, B, use_ld)
    v, s = (scalar(x, use_ld) for x in rice_vs(K))
    return v + s * z1, s * z2, s * z1


def rician_fading(N, K, seed, word0, B, use_ld=None):
    re, im, _ = rician_parts(N, K, seed, word0, B, use_ld)
    return sqrt_ref(re * re + im * im)


# ---------------------------------------------------------------- any kind

def fading(kind, param, N, seed, word0, B, use_ld=None):
    """h [B][N] of words [word0, word0 + B) in the reference's number type."""
    if kind == "rayleigh_block":
        return block_fading(N, param, seed, word0, B, use_ld)
    if kind == "rayleigh_correlated":
        a, b, _, _ = correlated_gauss(N, param, seed, word0, B, use_ld)
        return spread(symbol_fading(a, b), N)
    assert kind == "rician", kind
    return rician_fading(N, param, seed, word0, B, use_ld)


# ---------------------------------------------------------------- the statistics' standard errors

def se_mean_h2(kind, param, N, B):
    """The standard error of the mean of h^2 over B words of N elements (E[h^2] = 1).
    block:      h^2 = -log u is Exp(1), variance 1, one draw per block: the mean weighs a block by
                its size, Var = sum size^2 / (B N^2).
    Rician:     h^2 / s^2 is noncentral chi-square, 2 degrees, lambda = v^2 / s^2: variance
                s^4 (4 + 4 lambda) = 4 s^4 + 4 s^2 v^2, independent elements.
    correlated: h_q^2 = (a_q^2 + b_q^2) / 2 with cov(a_q^2, a_r^2) = 2 rho^(2 |q - r|) (Isserlis),
                so cov(h_q^2, h_r^2) = rho^(2 |q - r|); symbol q counts once per element it fills."""
    if kind == "rayleigh_block":
        S = int(param)
        sizes = np.bincount(np.arange(N) // S)
        return math.sqrt(float((sizes.astype(np.float64) ** 2).sum()) / B) / N
    if kind == "rician":
        v, s = (float(x) for x in rice_vs(param))
        return math.sqrt((4 * s ** 4 + 4 * s * s * v * v) / (B * N))
    nq = (N + 1) // 2
    wts = np.bincount(np.arange(N) // 2).astype(np.float64)
    q = np.arange(nq)
    cov = float(param) ** (2.0 * abs(q[:, None] - q[None, :]))
    return math.sqrt(float(wts @ cov @ wts) / B) / N


def lag1_estimate(h2q):
    """The lag-1 sample correlation of X_q = h_q^2 ([B][nq]) about the population mean 1 and
    variance 1 the model has by construction: the mean of (X_q - 1)(X_{q+1} - 1) over the pairs
    inside a word. Its expectation is cov(X_q, X_{q+1}) = rho^2 exactly."""
    z = np.asarray(h2q, np.float64) - 1.0
    return float((z[:, :-1] * z[:, 1:]).mean())


def se_lag1(rho, nq, B):
    """The standard error of lag1_estimate. Z_q = X_q - 1 = (A_q + B_q) / 2 with A_q = a_q^2 - 1:
    the joint cumulants of squares of unit Gaussians with correlations r_ij = rho^|i-j| are
    k2(A_i, A_j) = 2 r_ij^2 and k4(A_i, A_j, A_k, A_l) = 16 (r_ij r_jk r_kl r_li + r_ij r_jl r_lk r_ki
    + r_ik r_kj r_jl r_li) (the three 4-cycles); a and b are independent, so the cumulants of Z are
    2 (1/2)^n times those: k2 = r_ij^2, k4 = 2 (the three cycles). Z is centred, hence
    E[Z_i Z_j Z_k Z_l] = k4 + k2(ij) k2(kl) + k2(ik) k2(jl) + k2(il) k2(jk), and with Y_q = Z_q Z_{q+1}
    cov(Y_q, Y_r) = E[Z_q Z_{q+1} Z_r Z_{r+1}] - rho^4. Words are independent:
    Var = sum_{q, r} cov(Y_q, Y_r) / (B P^2), P = nq - 1 pairs a word."""
    P_ = nq - 1
    q = np.arange(P_)
    i, j = q[:, None], q[:, None] + 1
    k, l = q[None, :], q[None, :] + 1
    r = lambda x, y: float(rho) ** np.abs(x - y).astype(np.float64)  # noqa: E731
    k4 = 2.0 * (r(i, j) * r(j, k) * r(k, l) * r(l, i) + r(i, j) * r(j, l) * r(l, k) * r(k, i)
                + r(i, k) * r(k, j) * r(j, l) * r(l, i))
    k2 = lambda x, y: r(x, y) ** 2  # noqa: E731
    m4 = k4 + k2(i, j) * k2(k, l) + k2(i, k) * k2(j, l) + k2(i, l) * k2(j, k)
    cov = m4 - float(rho) ** 4
    return math.sqrt(float(cov.sum()) / B) / P_


def to_double(a):
    a = np.asarray(a)
    if a.dtype == object:
        return np.array([float(v) for v in a.ravel()], np.float64).reshape(a.shape)
    return a.astype(np.float64)

