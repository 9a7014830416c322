"""CPU reference of the fading / crossover uniform of the polar channel front-end
(bchk_polar_generate_channel_device), beside tests/philox_lib.py, which it extends and leaves as
it is.

Written from the comments of csrc/bchk_philox.h and include/bchk.h, not from the kernel: flat
element G = w N + position of a (seed, word) stream takes u(G) = v 2^-53, v in [1, 2^53], from
the Philox4x32-10 call with counter (G / 2 low, G / 2 high, 0xFAD1, 0) under the key (seed low,
seed high) -- unit53 of output words (0, 1) when G is even, of (2, 3) when G is odd. The Rayleigh
factor h = sqrt(-log u) is evaluated in philox_lib's number type above double (np.longdouble
with a 64-bit significand, or 50-digit Decimal on DEC_WORDS words where longdouble is a double).

Only tests/ import this.
"""
from decimal import Decimal, localcontext

import numpy as np

import philox_lib as P

TAG_UNIFORM = 0xFAD1
assert TAG_UNIFORM not in (P.TAG_INFO, P.TAG_NOISE, P.TAG_BEC)

AWGN, RAYLEIGH, BSC = 0, 1, 2
CHANNELS = {"awgn": AWGN, "rayleigh": RAYLEIGH, "bsc": BSC}


def element_units(first, count, seed):
    """v (uint64 [count], each in [1, 2^53]) of the flat stream elements [first, first + count):
    u = v 2^-53 in (0, 1]."""
    p0, p1 = first >> 1, (first + count - 1) >> 1
    pairs = np.arange(p1 - p0 + 1, dtype=np.uint64) + np.uint64(p0)
    lo, hi = P._split64(pairs)
    r = P.philox4x32_10((lo, hi, TAG_UNIFORM, 0), (seed & 0xFFFFFFFF, seed >> 32))
    v = np.stack([P.unit53_int(r[0], r[1]), P.unit53_int(r[2], r[3])], axis=1).reshape(-1)
    off = first - 2 * p0
    return v[off:off + count]


def word_units(N, seed, word0, B):
    """v [B][N] of words [word0, word0 + B) of a code of transmitted length N."""
    return element_units(word0 * N, B * N, seed).reshape(B, N)


def fading_from_units(v, use_ld=None):
    """h = sqrt(-log(v 2^-53)) in the reference's number type (0 at v = 2^53)."""
    v = np.asarray(v, dtype=np.uint64)
    if P.HAVE_LD if use_ld is None else use_ld:
        u = v.astype(np.longdouble) / np.longdouble(2.0 ** 53)  # exact: 54 bits at most
        return np.sqrt(-np.log(u))
    out = []
    with localcontext() as ctx:
        ctx.prec = P.DEC_PREC + 10
        for x in v.ravel().tolist():
            out.append((-(Decimal(x) / Decimal(1 << 53)).ln()).sqrt() if x != 1 << 53 else Decimal(0))
    return np.array(out, dtype=object).reshape(v.shape)


def bsc_flips(v, p):
    """The positions the BSC flips: u <= p, compared exactly (u = v 2^-53 is a double)."""
    return np.asarray(v, np.uint64).astype(np.float64) * 2.0 ** -53 <= np.float64(p)


def rayleigh_words(cw, N, K, snr, seed, word0, use_ld=None):
    """(h_ref [R][N], y_ref [R][N], noise [R][N] = sigma z_ref) for the sent codewords cw [B][N]:
    y = h x + sigma z with x = +1 for bit 1, sigma the double of philox_lib.polar_sigma, z the
    AWGN stream's element noise. R = B on the longdouble path, min(B, DEC_WORDS) on the decimal
    one."""
    B = len(cw)
    ld = P.HAVE_LD if use_ld is None else use_ld
    R = B if ld else min(B, P.DEC_WORDS)
    h = fading_from_units(word_units(N, seed, word0, R), ld)
    z = P.element_noise(word0 * N, R * N, seed, ld).reshape(R, N)
    noise = P.lift(np.float64(P.polar_sigma(N, K, snr)), ld) * z
    x = P.lift(np.where(np.asarray(cw)[:R] != 0, 1.0, -1.0), ld)
    return h, h * x + noise, noise
