// polar_channel.hip -- the simulation front-end of the polar SC-list decoder: the BPSK part of
// the vendored simulator's iteration (out/external/Simulator.cpp:104-114, :139-335,
// headers/external/Modem.h:64-78) over its three channels (:179-191: AWGN, real Rayleigh
// fading with ideal channel knowledge, the BSC) as batched kernels, so that a FER experiment
// never leaves the device. The words are statistically the simulator's (uniform information
// bits, Gaussian noise of its standard deviation, its Rayleigh factor, its flips), drawn from
// the counter-based generator of bchk_philox.h instead of its sequential GSL stream: word w of
// a (seed, channel parameter) stream depends only on (seed, w), and the information bits, the
// codeword and the Gaussian z of an element are the same on every channel.
//
// polar_gen_kernel: one wave per word, u as packed bits in LDS. CMixedKernelEncoder::Encode
// (out/external/MixedKernelEncoder.cpp:142-177): the information bits go to the unfrozen
// symbols (64 symbols per ballot), static frozen symbols are zeros, the dynamic constraints
// are walked in symbol order (a frozen symbol may depend on an earlier frozen one), their
// terms reduced across the lanes; then the layers, innermost first: an Arikan layer whose
// stride is a power of two is an XOR butterfly on the packed words, in place (shift and mask
// within a dword below 32, whole dwords above); any other layer is the l x l GF(2) product
// per block against the krows masks, 64 output symbols per ballot into the second buffer.
// The transmitted symbols are then stored as bytes, and (generate) element G = word * N +
// position of the stream takes one of the Box-Muller pair of counter G / 2. The kernel is a
// template over the channel: the Rayleigh and BSC instantiations draw one more uniform per
// element (the pair of counter G / 2 under the tag 0xFAD1) in the same loop, and every
// instantiation stores one LLR per symbol, h and y as doubles beside it when asked. Three more
// instantiations are the vendored library's fading models with a parameter
// (headers/external/Simulation/RayleighBlockChannel.h, RayleighCorrelatedChannel.h,
// RacianChannel.h; polar_device.h states them): block and Rician fading element-wise in the same
// loop, correlated fading in gen_correlated, whose recursion along the word runs across the lanes.
//
// polar_count_kernel: one wave per decoded word, CSimulator::Iterate's counters
// (Simulator.cpp:201-318); CurCorr and MLCorr of an errored word are summed in double in
// index order, as the reference forms them, so that its `>=` is reproduced.
#include <hip/hip_runtime.h>

#include "bchk_philox.h"
#include "polar_device.h"
#include "polar_enc_device.h"

namespace bchk {

namespace {

using penc::ubit;
using plist::wsync;

// One element of a fading channel: y = h x + sigma z (Simulator.cpp:185-186) and the LLR
// (Modem.h:78 with the fading factor), evaluated as ((-2 h) y) / var.
__device__ __forceinline__ void store_faded(const PolarGenParams &p, double fade, double x, double z, int el,
                                            float *llr, double *fout, double *yout) {
    const double y = fade * x + p.sigma * z;
    llr[el] = (float)(-2.0 * fade * y / p.var);
    if (fout) fout[el] = fade;
    if (yout) yout[el] = y;
}

// v of lane j (wave-uniform)
__device__ __forceinline__ double lane_f64(double v, int j) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)b >> 32), j);
    return __longlong_as_double((long long)((uint64_t)lo | ((uint64_t)hi << 32)));
}

// Correlated Rayleigh fading of one word (RayleighCorrelatedChannel.h:97-137): QAM symbol q =
// elements 2 q, 2 q + 1 of the word, 64 symbols at a time. Every lane draws the (z_a, z_b) of its
// symbol; the two AR(1) recursions (the Cholesky factor of rho^|i-j|) then walk the lanes in
// order, g carried in a register across the chunks -- the sequential recursion bit for bit, and
// nothing of it in LDS -- and every lane keeps the pair of its own step.
__device__ __forceinline__ void gen_correlated(const PolarGenParams &p, const uint32_t *c32, uint64_t word, int lane,
                                               float *llr, double *fout, double *yout) {
    const int N = p.t.N, nq = (N + 1) >> 1;
    const uint64_t ebase = word * (uint64_t)N;
    double ga = 0.0, gb = 0.0;  // wave-uniform; fma(rho, 0, z_0) = z_0
    for (int q0 = 0; q0 < nq; q0 += 64) {
        const int q = q0 + lane;
        double in[2] = {0.0, 0.0};
        if (q < nq) {
            normal_pair_of(word, kTagCorrelated, (uint32_t)q, p.seed_lo, p.seed_hi, in);
            if (q) {  // c z_q, rounded before the fma
                in[0] = p.f1 * in[0];
                in[1] = p.f1 * in[1];
            }
        }
        const int m = nq - q0 < 64 ? nq - q0 : 64;
        double a = 0.0, b = 0.0;
        for (int j = 0; j < m; ++j) {
            ga = fma(p.f0, ga, lane_f64(in[0], j));
            gb = fma(p.f0, gb, lane_f64(in[1], j));
            if (j == lane) {
                a = ga;
                b = gb;
            }
        }
        if (q < nq) {
            const double fade = sqrt((a * a + b * b) / 2.0);
            // z of the AWGN stream: flat elements g0 and g0 + 1 share a pair where g0 is even
            const uint64_t g0 = ebase + 2ull * (uint64_t)q;
            double z0[2], z1[2] = {0.0, 0.0};
            normal_pair(g0 >> 1, p.seed_lo, p.seed_hi, z0);
            if (g0 & 1ull) normal_pair((g0 >> 1) + 1ull, p.seed_lo, p.seed_hi, z1);  // wave-uniform
            const double zz[2] = {(g0 & 1ull) ? z0[1] : z0[0], (g0 & 1ull) ? z1[0] : z0[1]};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int el = 2 * q + h;
                if (el >= N) continue;
                const double x = ubit(c32, p.t.cwpos[el]) ? 1.0 : -1.0;
                store_faded(p, fade, x, zz[h], el, llr, fout, yout);
            }
        }
    }
}

template <int CH>
__global__ void __launch_bounds__(64 * kPolarChanWaves) polar_gen_kernel(PolarGenParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t psm[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const PolarEncTables &t = p.t;
    const int U = t.U, N = t.N, K = t.K;
    const int u64s = (U + 63) / 64, kq = 2 * ((K + 127) / 128) + 2;
    uint64_t *ib = reinterpret_cast<uint64_t *>(psm + (size_t)wid * polar_gen_wave_bytes(U, K));  // [kq]
    uint64_t *ua = ib + kq, *ub = ua + u64s;                                                       // [u64s] each
    const uint64_t nwaves = (uint64_t)gridDim.x * kPolarChanWaves;
    for (uint64_t w = (uint64_t)blockIdx.x * kPolarChanWaves + (uint64_t)wid; w < (uint64_t)p.B; w += nwaves) {
        const uint64_t word = p.word0 + w;
        // ---- information bits, packed: bit r of the word = bit r & 63 of ib[r >> 6]
        if (p.gen) {
            for (int blk = lane; blk * 128 < K; blk += 64) {
                const U4 r = philox(U4{(uint32_t)word, (uint32_t)(word >> 32), 0xFFFFFFFFu, (uint32_t)blk},
                                    p.seed_lo, p.seed_hi);
                ib[2 * blk] = (uint64_t)r.x | ((uint64_t)r.y << 32);
                ib[2 * blk + 1] = (uint64_t)r.z | ((uint64_t)r.w << 32);
            }
        } else {
            penc::pack_info(p.info_in + w * (uint64_t)K, K, ib, lane);
        }
        wsync();
        if (p.gen && p.info) {
            uint8_t *out = p.info + w * (uint64_t)K;
            for (int r = lane; r < K; r += 64) out[r] = (uint8_t)((ib[r >> 6] >> (r & 63)) & 1ull);
        }
        // ---- u: information bits at the unfrozen symbols, zeros at the static frozen ones, the
        // dynamic frozen symbols in symbol order (polar_enc_device.h)
        penc::build_u(t, ib, ua, lane);
        // ---- the transform, innermost layer first (MixedKernelEncoder.cpp:159-170): each block
        // of `next` symbols, viewed as l rows of `stride`, becomes (rows) x K
        uint64_t *src = ua, *dst = ub;
        for (int layer = t.nl - 1, stride = 1; layer >= 0; --layer) {
            const int l = t.ksize[layer], next = stride * l;
            const uint64_t *kr = t.krows + (size_t)layer * kPolarMaxKernel;
            uint32_t *s32 = reinterpret_cast<uint32_t *>(src);
            if (l == 2 && kr[0] == 1ull && kr[1] == 3ull && (stride & (stride - 1)) == 0) {
                // Arikan: u[b] ^= u[b + stride] where (b & stride) == 0
                if (stride < 32) {
                    const uint32_t M = stride == 1 ? 0x55555555u : stride == 2 ? 0x33333333u
                                     : stride == 4 ? 0x0F0F0F0Fu : stride == 8 ? 0x00FF00FFu : 0x0000FFFFu;
                    for (int d = lane; d < 2 * u64s; d += 64) {
                        const uint32_t x = s32[d];
                        s32[d] = x ^ ((x >> stride) & M);
                    }
                } else {  // U is a multiple of 2 stride >= 64
                    const int sd = stride >> 5, pairs = U >> 6;
                    for (int q = lane; q < pairs; q += 64) {
                        const int d = (q / sd) * 2 * sd + (q % sd);
                        s32[d] ^= s32[d + sd];
                    }
                }
            } else {
                for (int g = 0; g < u64s; ++g) {
                    const int pos = g * 64 + lane;
                    uint32_t acc = 0;
                    if (pos < U) {
                        const int b0 = pos / next * next, rem = pos - b0, i = rem / stride, s2 = rem - i * stride;
                        for (int j = 0; j < l; ++j)
                            if ((kr[j] >> i) & 1ull) acc ^= ubit(s32, b0 + j * stride + s2);
                    }
                    const uint64_t m = __ballot(acc != 0);
                    if (lane == 0) dst[g] = m;
                }
                uint64_t *tmp = src;
                src = dst;
                dst = tmp;
            }
            wsync();
            stride = next;
        }
        // ---- the transmitted symbols, and LLR = -2 y / var of y = BPSK + sigma z (AWGN); the
        // other channels: Simulator.cpp:183-191
        const uint32_t *c32 = reinterpret_cast<const uint32_t *>(src);
        if (p.cw) {
            uint8_t *cw = p.cw + w * (uint64_t)N;
            for (int i = lane; i < N; i += 64) cw[i] = (uint8_t)ubit(c32, t.cwpos[i]);
        }
        if (p.gen) {
            // global element G = word * N + position; the Box-Muller pair of counter G / 2 gives
            // elements 2 p and 2 p + 1 (a pair may straddle two words: each wave computes it),
            // and so does the pair of fading / crossover uniforms
            float *llr = p.llr + w * (uint64_t)N;
            double *fout = (CH == kPolarChanRayleigh || CH >= kPolarChanFading) && p.fade ? p.fade + w * (uint64_t)N
                                                                                           : nullptr;
            double *yout = p.y ? p.y + w * (uint64_t)N : nullptr;
            const uint64_t ebase = word * (uint64_t)N;
            const uint64_t p0 = ebase >> 1, pend = (ebase + (uint64_t)N + 1) >> 1;
            if constexpr (CH == kPolarChanCorrelated) {  // the recursion along the word: a loop of its own
                gen_correlated(p, c32, word, lane, llr, fout, yout);
            } else {
                for (uint64_t pr = p0 + (uint64_t)lane; pr < pend; pr += 64) {
                    double z[2], u[2];
                    if (CH != kPolarChanBsc) normal_pair(pr, p.seed_lo, p.seed_hi, z);
                    if (CH == kPolarChanRayleigh || CH == kPolarChanBsc) unit_pair(pr, p.seed_lo, p.seed_hi, u);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int64_t el = (int64_t)(2 * pr + (uint64_t)h) - (int64_t)ebase;  // within the word
                        if (el < 0 || el >= (int64_t)N) continue;
                        const double x = ubit(c32, t.cwpos[el]) ? 1.0 : -1.0;  // Modem.h:64
                        if constexpr (CH == kPolarChanAwgn) {
                            const double y = x + p.sigma * z[h];
                            llr[el] = (float)(-2.0 * y / p.var);  // Modem.h:78
                            if (yout) yout[el] = y;
                        } else if constexpr (CH == kPolarChanRayleigh) {
                            // gsl_ran_rayleigh(1 / sqrt 2), Simulator.cpp:184-186
                            store_faded(p, sqrt(-log(u[h])), x, z[h], (int)el, llr, fout, yout);
                        } else if constexpr (CH == kPolarChanBlock) {
                            // the Rayleigh factor of the first element of the block (RayleighBlockChannel.h:61-70)
                            const uint64_t gb = ebase + (uint64_t)((int)el / p.fblock) * (uint64_t)p.fblock;
                            double ub[2];
                            unit_pair(gb >> 1, p.seed_lo, p.seed_hi, ub);
                            store_faded(p, sqrt(-log(ub[gb & 1ull])), x, z[h], (int)el, llr, fout, yout);
                        } else if constexpr (CH == kPolarChanRician) {
                            // Rice(v, s): the line-of-sight part v on the first of two N(0, s^2) components
                            double r[2];
                            normal_pair_of(word, kTagRician, (uint32_t)el, p.seed_lo, p.seed_hi, r);
                            const double re = p.f0 + p.f1 * r[0], im = p.f1 * r[1];
                            store_faded(p, sqrt(re * re + im * im), x, z[h], (int)el, llr, fout, yout);
                        } else {
                            const double y = u[h] > p.cross ? x : -x;  // :189-190
                            llr[el] = (float)(-2.0 * y);  // noise variance 1 (:114)
                            if (yout) yout[el] = y;
                        }
                    }
                }
            }
        }
        wsync();  // the next word overwrites the buffers
    }
}

__global__ void __launch_bounds__(64 * kPolarChanWaves) polar_count_kernel(PolarCountParams p) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int N = p.N, K = p.K, L = p.L;
    unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // wave-uniform
    const uint64_t nwaves = (uint64_t)gridDim.x * kPolarChanWaves;
    for (uint64_t w = (uint64_t)blockIdx.x * kPolarChanWaves + (uint64_t)wid; w < (uint64_t)p.B; w += nwaves) {
        const float *llr = p.llr + w * (uint64_t)N;
        const uint8_t *ctx = p.cw_tx + w * (uint64_t)N, *itx = p.info_tx + w * (uint64_t)K;
        const uint8_t *info0 = p.info + w * (uint64_t)L * (uint64_t)K, *cw0 = p.cw + w * (uint64_t)L * (uint64_t)N;
        int cnt = p.count[w];
        if (cnt > L) cnt = L;
        // raw bit errors (:203-208)
        uint32_t raw = 0;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;
            bool e = false;
            if (i < N) {
                const float v = llr[i];
                e = (ctx[i] ? -v : v) < 0.0f;
            }
            raw += (uint32_t)__popcll(__ballot(e));
        }
        c[0] += 1;
        c[6] += raw;
        uint32_t fl = 0;
        if (cnt <= 0) {  // no decision: a block and list error; nothing to compare
            c[1] += 1;
            c[5] += 1;
            c[7] += 1;
            fl = 1u | 4u;
        } else {
            uint32_t ibe = 0, cbe = 0;  // row 0 against the sent word (:245-254)
            for (int i0 = 0; i0 < K; i0 += 64) {
                const int i = i0 + lane;
                ibe += (uint32_t)__popcll(__ballot(i < K && ((info0[i] != 0) != (itx[i] != 0))));
            }
            if (ibe) {
                for (int i0 = 0; i0 < N; i0 += 64) {
                    const int i = i0 + lane;
                    cbe += (uint32_t)__popcll(__ballot(i < N && ((cw0[i] != 0) != (ctx[i] != 0))));
                }
                c[1] += 1;
                c[2] += ibe;
                c[3] += cbe;
                fl = 1u;
                // MLCorr / CurCorr (:265-271): double sums of +-llr in index order
                double ml = 0.0, cur = 0.0;
                for (int i0 = 0; i0 < N; i0 += 64) {
                    const int i = i0 + lane;
                    const float v = i < N ? llr[i] : 0.0f;
                    const uint64_t mt = __ballot(i < N && ctx[i] != 0), md = __ballot(i < N && cw0[i] != 0);
                    const int m = N - i0 < 64 ? N - i0 : 64;
                    for (int j = 0; j < m; ++j) {
                        const float vj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
                        ml += (double)(((mt >> j) & 1ull) ? -vj : vj);
                        cur += (double)(((md >> j) & 1ull) ? -vj : vj);
                    }
                }
                if (cur >= ml) {  // :286
                    c[4] += 1;
                    fl |= 2u;
                }
                bool found = false;  // the sent codeword among rows 1 .. count - 1 (:288-305)
                for (int r = 1; r < cnt && !found; ++r) {
                    const uint8_t *row = cw0 + (size_t)r * (size_t)N;
                    bool diff = false;
                    for (int i0 = 0; i0 < N && !diff; i0 += 64) {
                        const int i = i0 + lane;
                        diff = __ballot(i < N && ((row[i] != 0) != (ctx[i] != 0))) != 0ull;
                    }
                    found = !diff;
                }
                if (!found) {
                    c[5] += 1;
                    fl |= 4u;
                }
            }
        }
        if (p.flags && lane == 0) p.flags[w] = (uint8_t)fl;
    }
    if (lane == 0)
        for (int q = 0; q < 8; ++q)
            if (c[q]) atomicAdd(p.out8 + q, c[q]);
}

int chan_grid(uint32_t B) {
    const uint32_t blocks = (B + kPolarChanWaves - 1) / kPolarChanWaves;
    return (int)(blocks < 2048u ? blocks : 2048u);  // the waves stride over the rest
}

}  // namespace

hipError_t launch_polar_gen(const PolarGenParams &p, hipStream_t s) {
    if (p.B == 0) return hipSuccess;
    const size_t lds = (size_t)kPolarChanWaves * polar_gen_wave_bytes(p.t.U, p.t.K);  // <= 25 KiB at U = K = 16384
    const dim3 grid(chan_grid(p.B)), block(64 * kPolarChanWaves);
    if (p.gen && p.channel == kPolarChanRayleigh)
        hipLaunchKernelGGL(polar_gen_kernel<kPolarChanRayleigh>, grid, block, lds, s, p);
    else if (p.gen && p.channel == kPolarChanBsc)
        hipLaunchKernelGGL(polar_gen_kernel<kPolarChanBsc>, grid, block, lds, s, p);
    else if (p.gen && p.channel == kPolarChanBlock)
        hipLaunchKernelGGL(polar_gen_kernel<kPolarChanBlock>, grid, block, lds, s, p);
    else if (p.gen && p.channel == kPolarChanCorrelated)
        hipLaunchKernelGGL(polar_gen_kernel<kPolarChanCorrelated>, grid, block, lds, s, p);
    else if (p.gen && p.channel == kPolarChanRician)
        hipLaunchKernelGGL(polar_gen_kernel<kPolarChanRician>, grid, block, lds, s, p);
    else  // AWGN, and every encode
        hipLaunchKernelGGL(polar_gen_kernel<kPolarChanAwgn>, grid, block, lds, s, p);
    return hipGetLastError();
}

hipError_t launch_polar_count(const PolarCountParams &p, hipStream_t s) {
    if (p.B == 0) return hipSuccess;
    hipLaunchKernelGGL(polar_count_kernel, dim3(chan_grid(p.B)), dim3(64 * kPolarChanWaves), 0, s, p);
    return hipGetLastError();
}

}  // namespace bchk
