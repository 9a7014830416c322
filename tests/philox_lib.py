"""CPU reference of the counter-based channel streams (csrc/bchk_philox.h and its three users:
chan_kernel, polar_gen_kernel, draw_rank), in numpy and Python integers.

Written from the documentation, not from the kernels: Philox4x32-10 from the round description
of Salmon et al. (SC'11), the counter layouts from the comments of csrc/bchk_philox.h and
include/bchk.h, Box-Muller in a precision well above double. The Gaussian pair is evaluated in
np.longdouble where that has a 64-bit significand (x86), with the angle reduced exactly in
integers so the trigonometric functions only see [0, pi/4]; a 50-digit `decimal` evaluation
(Decimal.ln, Decimal.sqrt, Taylor series) checks it, and replaces it on a smaller sample where
np.longdouble is only a double.

Only tests/ import this.
"""
import math
from decimal import Decimal, localcontext

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57   # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # the Weyl increments of the key
TAG_INFO, TAG_NOISE, TAG_BEC = 0xFFFFFFFF, 0x5EED, 0xBEC00000
MASK32 = np.uint64(0xFFFFFFFF)

HAVE_LD = np.finfo(np.longdouble).nmant >= 63
DEC_PREC = 50
DEC_WORDS = 6  # words of a batch that get a noise reference on the decimal path
PI_DEC = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")
PI_LD = np.longdouble("3.14159265358979323846264338327950288419716939937510") if HAVE_LD else None


# ---------------------------------------------------------------- Philox4x32-10

def _u64(a):
    return np.atleast_1d(np.asarray(a)).astype(np.uint64) & MASK32


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (scalars or arrays, broadcast together) -> 4 uint32
    arrays. One round maps (c0, c1, c2, c3) under (k0, k1) to
    (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped by the
    Weyl constants between rounds."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) for c in counter])
    k0, k1 = _u64(key[0]), _u64(key[1])
    for rnd in range(10):
        if rnd:
            k0 = (k0 + np.uint64(W0)) & MASK32
            k1 = (k1 + np.uint64(W1)) & MASK32
        p0 = np.uint64(M0) * c0  # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _split64(v):
    v = np.atleast_1d(np.asarray(v, dtype=np.uint64))
    return v & MASK32, v >> np.uint64(32)


def unit53_int(a, b):
    """v + 1 of unit53: the integer in [1, 2^53] whose 2^-53 multiple is the uniform."""
    a, b = np.asarray(a).astype(np.uint64), np.asarray(b).astype(np.uint64)
    return (a << np.uint64(21)) + (b >> np.uint64(11)) + np.uint64(1)


def unit53(a, b):
    """(a 2^21 + (b >> 11) + 1) 2^-53 in (0, 1], exact in double."""
    return unit53_int(a, b).astype(np.float64) * 2.0 ** -53


# ---------------------------------------------------------------- Box-Muller above double

def _octant(v2):
    """2 pi u2 with u2 = v2 2^-53 as (octant 0..7, r) with the angle inside the octant folded
    to theta = r pi / 2^52 in [0, pi/4], r an integer in [0, 2^50]."""
    v2 = int(v2)
    octant, r = (v2 >> 50) & 7, v2 & ((1 << 50) - 1)
    if octant & 1:
        r = (1 << 50) - r
    return octant, r


# (cos, sin) of the full angle from (c, s) = (cos theta, sin theta): (which, sign) per octant
_COS = [("c", 1), ("s", 1), ("s", -1), ("c", -1), ("c", -1), ("s", -1), ("s", 1), ("c", 1)]
_SIN = [("s", 1), ("c", 1), ("c", 1), ("s", 1), ("s", -1), ("c", -1), ("c", -1), ("s", -1)]


def normal_from_units_ld(v1, v2):
    """(z0, z1) in np.longdouble for the uniforms u1 = v1 2^-53, u2 = v2 2^-53 (v in [1, 2^53])."""
    assert HAVE_LD
    v1 = np.atleast_1d(np.asarray(v1, dtype=np.uint64))
    v2 = np.atleast_1d(np.asarray(v2, dtype=np.uint64))
    two53 = np.longdouble(2.0 ** 53)
    u1 = v1.astype(np.longdouble) / two53  # exact: 54 bits at most
    rad = np.sqrt(np.longdouble(-2.0) * np.log(u1))
    octant = ((v2 >> np.uint64(50)) & np.uint64(7)).astype(np.int64)
    r = v2 & np.uint64((1 << 50) - 1)
    r = np.where(octant & 1, np.uint64(1 << 50) - r, r)
    theta = r.astype(np.longdouble) * (PI_LD / np.longdouble(2.0 ** 52))
    c, s = np.cos(theta), np.sin(theta)
    pick = {"c": c, "s": s}
    cosv, sinv = np.zeros_like(c), np.zeros_like(c)
    for o in range(8):
        m = octant == o
        cosv[m] = pick[_COS[o][0]][m] * _COS[o][1]
        sinv[m] = pick[_SIN[o][0]][m] * _SIN[o][1]
    return rad * cosv, rad * sinv


def _sincos_dec(theta):
    """Taylor series of (cos, sin) for a Decimal 0 <= theta <= pi/4 in the current context."""
    t2 = theta * theta
    c = term = Decimal(1)
    k = 0
    while True:
        k += 2
        term = -term * t2 / ((k - 1) * k)
        if abs(term) < Decimal(10) ** -(DEC_PREC + 8):
            break
        c += term
    s = term = theta
    k = 1
    while theta:
        k += 2
        term = -term * t2 / ((k - 1) * k)
        if abs(term) < Decimal(10) ** -(DEC_PREC + 8) * abs(theta):
            break
        s += term
    return c, s


def normal_from_units_dec(v1, v2):
    """The same pair for one (v1, v2), as Decimals of DEC_PREC digits (series terms carried
    with 10 digits more)."""
    with localcontext() as ctx:
        ctx.prec = DEC_PREC + 10
        u1 = Decimal(int(v1)) / Decimal(1 << 53)
        rad = (Decimal(-2) * u1.ln()).sqrt()
        octant, r = _octant(v2)
        c, s = _sincos_dec(Decimal(r) * PI_DEC / Decimal(1 << 52))
        pick = {"c": c, "s": s}
        z0 = rad * pick[_COS[octant][0]] * _COS[octant][1]
        z1 = rad * pick[_SIN[octant][0]] * _SIN[octant][1]
        ctx.prec = DEC_PREC
        return +z0, +z1


def ld_to_decimal(x):
    """Exact Decimal of one np.longdouble."""
    m, e = np.frexp(np.longdouble(x))
    hi = np.floor(m * np.longdouble(2.0 ** 32))
    lo = (m * np.longdouble(2.0 ** 32) - hi) * np.longdouble(2.0 ** 32)
    mant = int(float(hi)) * (1 << 32) + int(float(lo))  # m 2^64 as an integer
    with localcontext() as ctx:
        ctx.prec = 200
        e = int(e) - 64
        return Decimal(mant) * (Decimal(2) ** e if e >= 0 else Decimal(1) / Decimal(2) ** -e)


def pair_units(pair, seed):
    """(v1, v2) of noise counter `pair` (uint64 array): counter (pair low, pair high, 0x5EED, 0),
    key (seed low, seed high); u1 from output words (0, 1), u2 from (2, 3)."""
    lo, hi = _split64(pair)
    r = philox4x32_10((lo, hi, TAG_NOISE, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return unit53_int(r[0], r[1]), unit53_int(r[2], r[3])


def normal_pair(pair, seed, use_ld=None):
    """(z0, z1) of noise counters `pair`: rad = sqrt(-2 ln u1), z0 = rad cos(2 pi u2), z1 = rad
    sin(2 pi u2). np.longdouble arrays, or object arrays of Decimal where longdouble is a double
    (or use_ld is False)."""
    v1, v2 = pair_units(pair, seed)
    if HAVE_LD if use_ld is None else use_ld:
        return normal_from_units_ld(v1, v2)
    z = [normal_from_units_dec(a, b) for a, b in zip(v1.tolist(), v2.tolist())]
    return (np.array([p[0] for p in z], dtype=object), np.array([p[1] for p in z], dtype=object))


def lift(a, use_ld=None):
    """A double / integer array in the reference's number type (exact)."""
    if HAVE_LD if use_ld is None else use_ld:
        return np.asarray(a).astype(np.longdouble)
    a = np.asarray(a)
    return np.array([Decimal(v) for v in a.ravel().tolist()], dtype=object).reshape(a.shape)


def element_noise(first, count, seed, use_ld=None):
    """z of the flat stream elements [first, first + count): element G takes z[G & 1] of pair
    G >> 1."""
    p0, p1 = first >> 1, (first + count - 1) >> 1
    pairs = np.arange(p1 - p0 + 1, dtype=np.uint64) + np.uint64(p0)
    z0, z1 = normal_pair(pairs, seed, use_ld)
    z = np.stack([z0, z1], axis=1).reshape(-1)
    off = first - 2 * p0
    return z[off:off + count]


# ---------------------------------------------------------------- the BCH stream

def info_block_words(words, block_word3, seed):
    """The four output words [4][B] of the information-bit call of `words` (uint64 [B])."""
    lo, hi = _split64(words)
    return np.stack(philox4x32_10((lo, hi, TAG_INFO, block_word3), (seed & 0xFFFFFFFF, seed >> 32)))


def bch_sd(n, k, snr):
    return math.sqrt(1 / (10 ** (snr / 10) * 2 * k / n))  # src/dataForPlot.cpp:45


def bch_words(g, n, k, snr, seed, word0, B, use_ld=None):
    """Words [word0, word0 + B) of the BCH stream: (tx [B][n] u8, y_ref [R][n], z_ref [R][n])
    in the reference's number type, R = B (longdouble) or min(B, DEC_WORDS) (decimal).
    Coefficient i of info(x) is bit (i % 128) & 31 of output word (i % 128) >> 5 of the call
    with counter (w low, w high, 0xFFFFFFFF, 128 (i // 128)) -- the BCH stream's counter word 3
    is the bit offset of the 128-bit block. tx = info(x) g(x) over GF(2)."""
    g = np.asarray(g, np.uint8)
    assert len(g) == n - k + 1
    words = np.arange(B, dtype=np.uint64) + np.uint64(word0)
    info = np.zeros((B, k), np.uint8)
    for blk in range((k + 127) // 128):
        r = info_block_words(words, 128 * blk, seed)
        for i in range(128 * blk, min(k, 128 * blk + 128)):
            q = i % 128
            info[:, i] = (r[q >> 5] >> np.uint32(q & 31)) & np.uint32(1)
    tx = np.zeros((B, n), np.uint8)
    for i in range(k):
        tx[:, i:i + len(g)] ^= info[:, i:i + 1] * g[None, :]
    ld = HAVE_LD if use_ld is None else use_ld
    R = B if ld else min(B, DEC_WORDS)
    z = element_noise(word0 * n, R * n, seed, ld).reshape(R, n)
    sd = lift(np.float64(bch_sd(n, k, snr)), ld)
    y = lift(np.where(tx[:R] != 0, 1.0, -1.0), ld) + sd * z
    return tx, y, z


# ---------------------------------------------------------------- the polar stream

def polar_sigma(N, K, snr):
    return math.sqrt(0.5 * 10.0 ** (-snr / 10.0) * N / K)  # Simulator.cpp:108


def polar_info(K, seed, word0, B):
    """Information bits [B][K]: bit r is bit r & 63 of (x | y << 32) for even 64-bit halves,
    (z | w << 32) for odd ones, of block r // 128 -- the call with counter
    (w low, w high, 0xFFFFFFFF, block index)."""
    words = np.arange(B, dtype=np.uint64) + np.uint64(word0)
    info = np.zeros((B, K), np.uint8)
    for blk in range((K + 127) // 128):
        r = [a.astype(np.uint64) for a in info_block_words(words, blk, seed)]
        halves = [r[0] | (r[1] << np.uint64(32)), r[2] | (r[3] << np.uint64(32))]
        for i in range(128 * blk, min(K, 128 * blk + 128)):
            info[:, i] = (halves[(i >> 6) & 1] >> np.uint64(i & 63)) & np.uint64(1)
    return info


def polar_words(encode, N, K, snr, seed, word0, B, use_ld=None):
    """(info [B][K], cw [B][N], llr_ref [R][N]) with cw = encode(info) (PolarOracle.encode),
    x = +1 for bit 1, y = x + sigma z, LLR = -2 y / sigma^2 in the reference's number type;
    sigma and sigma^2 are the doubles the host forms."""
    info = polar_info(K, seed, word0, B)
    cw = np.asarray(encode(info), np.uint8)
    assert cw.shape == (B, N)
    ld = HAVE_LD if use_ld is None else use_ld
    R = B if ld else min(B, DEC_WORDS)
    sigma = np.float64(polar_sigma(N, K, snr))
    var = sigma * sigma
    z = element_noise(word0 * N, R * N, seed, ld).reshape(R, N)
    y = lift(np.where(cw[:R] != 0, 1.0, -1.0), ld) + lift(sigma, ld) * z
    return info, cw, lift(np.float64(-2.0), ld) * y / lift(var, ld)


def _to_f32(a):
    a = np.asarray(a)
    if a.dtype == object:  # Decimal -> double (correctly rounded) -> float32: monotone
        return np.array([float(v) for v in a.ravel()], np.float64).reshape(a.shape).astype(np.float32)
    return a.astype(np.float32)


def llr_float32(llr_ref):
    """(expected float32, decidable): an element is decidable when every double within 2^-48
    relative of the reference rounds to the same float32 (the decimal path adds the 2^-53 of
    its own detour through double to the interval)."""
    a = np.asarray(llr_ref)
    rel = lift(np.float64(2.0 ** -48 + (0.0 if a.dtype != object else 2.0 ** -52)), a.dtype != object)
    one = lift(np.float64(1.0), a.dtype != object)
    lo, hi = _to_f32(a * (one - rel)), _to_f32(a * (one + rel))
    return _to_f32(a), lo.view(np.uint32) == hi.view(np.uint32)


# ---------------------------------------------------------------- the sampled BEC design

def unrank_colex(l, w, r):
    """The w-subset of {0..l-1} of colex rank r as a bit mask: the largest element is the
    largest c with C(c, w) <= r, and so on down."""
    x, k = 0, w
    for c in range(l - 1, -1, -1):
        if k == 0:
            break
        b = math.comb(c, k)
        if r >= b:
            x |= 1 << c
            r -= b
            k -= 1
    assert k == 0 and r == 0
    return x


def bec_draw(l, w, seed, s):
    """include/bchk.h's rule for sample(s) `s` of weight w (bchk_kernel_bec_sample): 64-bit
    candidates (y << 32 | x) then (w << 32 | z) of counter (s low, s high, w, 0xBEC00000 +
    attempt), each masked to the bit length of C(l, w) - 1, the first one below C(l, w) taken.
    -> (patterns uint64 [S], ranks, attempts, candidates) -- the last three as Python lists:
    the rank, the attempt that produced it and which of its two candidates (0 / 1)."""
    s = np.atleast_1d(np.asarray(s, dtype=np.uint64))
    total = math.comb(l, w)
    assert total >= 2
    mask = (1 << (total - 1).bit_length()) - 1
    ranks, attempts, cands = [None] * len(s), [None] * len(s), [None] * len(s)
    pending = np.arange(len(s))
    for attempt in range(64):
        if not len(pending):
            break
        lo, hi = _split64(s[pending])
        r = philox4x32_10((lo, hi, w, TAG_BEC + attempt), (seed & 0xFFFFFFFF, seed >> 32))
        x, y, z, ww = (a.tolist() for a in r)
        still = []
        for j, idx in enumerate(pending.tolist()):
            for cand, v in enumerate(((y[j] << 32 | x[j]) & mask, (ww[j] << 32 | z[j]) & mask)):
                if v < total:
                    ranks[idx], attempts[idx], cands[idx] = v, attempt, cand
                    break
            else:
                still.append(idx)
        pending = np.array(still, dtype=np.int64)
    assert not len(pending)
    pats = np.array([unrank_colex(l, w, r) for r in ranks], dtype=np.uint64)
    return pats, ranks, attempts, cands
