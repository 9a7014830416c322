// bchk_philox.h -- the counter-based generator of the on-GPU channel front-ends
// (bchk_channel.hip for BCH words, polar_channel.hip for polar words) and of the sampled BEC
// design (kernel_bec.hip). Device code only.
//
// Counter layout of a (seed, word) stream, keyed by (seed low, seed high):
//   information bits of word w, 128 at a time:  (w low, w high, 0xFFFFFFFF, c3); bit q of the
//                                               block is bit q & 31 of output word q >> 5.
//       BCH stream (chan_kernel):               c3 = the bit offset of the block (0, 128)
//       polar stream (polar_gen_kernel):        c3 = the index of the block (0, 1, 2, ...)
//     The two differ from the second block on (only BCH(255,139) has one among the built-in
//     BCH codes). Both stay as they are: recorded profiles were produced with them, and the
//     two streams never share a counter, so neither is wrong -- only different.
//   noise of flat element G = w * n + position: element G & 1 of the Box-Muller pair of counter
//                                               (G / 2 low, G / 2 high, 0x5EED, 0): u1 from
//                                               output words (0, 1), u2 from (2, 3)
//   fading / crossover uniform u(G) of the same flat element G (polar stream, Rayleigh and BSC
//   channels):                                  counter (G / 2 low, G / 2 high, 0xFAD1, 0);
//                                               u = unit53 of output words (0, 1) when G is
//                                               even, of (2, 3) when G is odd: (a 2^21 + (b >> 11)
//                                               + 1) 2^-53 in (0, 1] for the word pair (a, b)
//   BEC pattern draw of sample s, weight w:     (s low, s high, w, 0xBEC00000 + attempt)
//   correlated fading, QAM symbol q of word w (polar stream): the Box-Muller pair of counter
//                                               (w low, w high, 0xC022, q): element 0 drives the
//                                               sequence a, element 1 the sequence b
//   Rician fading, position i of word w (polar stream): the Box-Muller pair (z1, z2) of counter
//                                               (w low, w high, 0x21CE, i)
// Word 2 tells the six apart: 0xFFFFFFFF, 0x5EED, 0xFAD1, 0xC022, 0x21CE, and a weight of at
// most 64.
// tests/philox_lib.py restates all of it but u(G), which tests/channel_lib.py restates, and the
// two fading pairs, which tests/fading_lib.py restates; tests/test_stream_reference.py,
// tests/test_polar_channels.py and tests/test_polar_fading.py compare.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bchk {

struct U4 {
    uint32_t x, y, z, w;
};

// Philox4x32-10 (Salmon et al., SC'11): 10 rounds of the 4x32 bijection keyed by (k0, k1)
__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(M0, c.x), l0 = M0 * c.x;
        const uint32_t h1 = __umulhi(M1, c.z), l1 = M1 * c.z;
        c = U4{h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0};
        k0 += W0;
        k1 += W1;
    }
    return c;
}

// (0, 1] with 53 random bits
__device__ __forceinline__ double unit53(uint32_t a, uint32_t b) {
    const uint64_t v = ((uint64_t)a << 21) ^ (uint64_t)(b >> 11);  // 53 bits
    return ((double)(v & ((1ull << 53) - 1ull)) + 1.0) * 0x1p-53;
}

constexpr uint32_t kTagCorrelated = 0xC022u, kTagRician = 0x21CEu;

// the standard normal pair (Box-Muller) of counter (c low, c high, tag, c3)
__device__ __forceinline__ void normal_pair_of(uint64_t c, uint32_t tag, uint32_t c3, uint32_t k0, uint32_t k1,
                                               double z[2]) {
    const U4 r = philox(U4{(uint32_t)c, (uint32_t)(c >> 32), tag, c3}, k0, k1);
    const double u1 = unit53(r.x, r.y), u2 = unit53(r.z, r.w);
    const double rad = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    z[0] = rad * cs;
    z[1] = rad * sn;
}

// the standard normal pair of noise counter `pair` (elements 2 pair and 2 pair + 1)
__device__ __forceinline__ void normal_pair(uint64_t pair, uint32_t k0, uint32_t k1, double z[2]) {
    normal_pair_of(pair, 0x5EEDu, 0u, k0, k1, z);
}

// the fading / crossover uniforms of counter `pair` (elements 2 pair and 2 pair + 1)
__device__ __forceinline__ void unit_pair(uint64_t pair, uint32_t k0, uint32_t k1, double u[2]) {
    const U4 r = philox(U4{(uint32_t)pair, (uint32_t)(pair >> 32), 0xFAD1u, 0u}, k0, k1);
    u[0] = unit53(r.x, r.y);
    u[1] = unit53(r.z, r.w);
}

}  // namespace bchk
