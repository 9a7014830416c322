// polar_sclist_q8.hip -- fixed-point SC-list decoding of all-Arikan polar codes on gfx950:
// polar_sclist_kernel (polar_sclist.hip) with int8 LLRs, and the quantiser that makes them.
//
// The arithmetic is the vendored library's USE_INT8 configuration (SeqConfigOrig.h:186-194,
// SoftProcessing.cpp:643-1146) with symmetric saturation; the contract is stated in
// include/bchk.h and DESIGN 5.18 and restated in tests/sclist_q8.py:
//   load   -128 reads as -127, a punctured symbol is 0, a shortened one +127
//   f      sgn(a) sgn(b) min(|a|, |b|)
//   g      clamp(u ? b - a : b + a, -127, +127)
//   metric a decision against the sign of v costs |v|
// A path metric is an integer of magnitude <= 127 U < 2^24, exact in an f32: the list
// bookkeeping (plist::, polar_list_device.h) is the f32 kernel's, called unchanged, with the leaf
// LLR and the metric held as floats. So are the packed C layout, cwoff, the partial-sum
// butterflies and the epilogues, restated here as in every list kernel.
//
// What is new is S: per path U - 1 bytes (polar_q8_layout), a quarter of the f32 kernel's. A
// layer of d >= 4 LLRs is processed four to a lane: one 32-bit LDS word per operand, the four
// known bits of a g step from one extract of the packed C word (s is a multiple of 4, so they
// never straddle a word). Layers of one or two LLRs go element by element. No MFMA, no inline
// assembly.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_list_device.h"

namespace bchk {

namespace {

using namespace plist;

// offset of S_λ (λ >= 1) inside one path's LLR bytes
__device__ __forceinline__ int s_off(int U, int lam) { return U - (U >> (lam - 1)); }

__device__ __forceinline__ int q8_clamp(int v) { return v > kQ8Max ? kQ8Max : (v < -kQ8Max ? -kQ8Max : v); }
// LoadLLRs on int8 rows
__device__ __forceinline__ int chan_q8(const int16_t *symmap, const int8_t *y, int i) {
    const int m = symmap[i];
    return m >= 0 ? q8_clamp((int)y[m]) : (m == -1 ? kQ8Max : 0);
}
__device__ __forceinline__ int q8_f(int a, int b) {
    const int ma = a < 0 ? -a : a, mb = b < 0 ? -b : b;
    const int m = ma < mb ? ma : mb;
    return ((a ^ b) < 0) ? -m : m;
}
__device__ __forceinline__ int q8_g(int a, int b, uint32_t u) { return q8_clamp(u ? b - a : b + a); }
// byte k of a packed word, sign-extended, and back
__device__ __forceinline__ int q8_at(uint32_t w, int k) { return (int)(int8_t)(uint8_t)(w >> (8 * k)); }
__device__ __forceinline__ uint32_t q8_put(int v, int k) { return ((uint32_t)v & 255u) << (8 * k); }
__device__ __forceinline__ uint32_t q8_f4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= q8_put(q8_f(q8_at(a, k), q8_at(b, k)), k);
    return r;
}
__device__ __forceinline__ uint32_t q8_g4(uint32_t a, uint32_t b, uint32_t u4) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= q8_put(q8_g(q8_at(a, k), q8_at(b, k), (u4 >> k) & 1u), k);
    return r;
}

}  // namespace

__global__ void __launch_bounds__(64) polar_sclist_q8_kernel(PolarQ8Params pq) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const PolarParams &p = pq.p;
    const int lane = (int)threadIdx.x;
    const int U = p.U, n = p.n, L = p.L, K = p.K;
    const int pathS = polar_path_q8(U), pathC = p.pathCw, RW = polar_rec_words(K);
    // LDS layout: polar_q8_layout (polar_device.h); byte offsets from smem, as in the f32 kernel
    const PolarListLayout lo = polar_q8_layout(U, L, K, pathC);
    int8_t *S = reinterpret_cast<int8_t *>(smem);
    uint32_t *C = reinterpret_cast<uint32_t *>(smem + lo.o_C);  // packed bits, words per path
    uint32_t *act = reinterpret_cast<uint32_t *>(smem + lo.o_act);
    uint32_t *rec = act + L;
    const int lastc = p.cwoff[n];  // C_n: the two inputs of the last Arikan block (one word)
    const bool mine = lane < L;

    PathStack st;
    st.slot = 0;
    for (uint32_t cw = blockIdx.x; cw < p.B; cw += gridDim.x) {
        const int8_t *y = pq.llr8 + (size_t)cw * p.N;
        auto chan = [&](int i) -> int { return chan_q8(p.io.symmap, y, i); };
        auto chan4 = [&](int i) -> uint32_t {
            return q8_put(chan(i), 0) | q8_put(chan(i + 1), 1) | q8_put(chan(i + 2), 2) | q8_put(chan(i + 3), 3);
        };
        // ---- Cleanup + AssignInitialPath (TVMemoryEngine.cpp:58-94)
        st.reset(L, lane);
        const uint32_t pid = st.pop(lane);
        uint32_t active = 1u << pid;
        PathRegs pr{0.0f, 0.0f, 0ull, 0u};
        int k = 0;  // unfrozen decisions so far
        wsync();
        int nact = list_active(active, act, lane, L);

        for (int phi = 0; phi < U; ++phi) {
            const uint32_t e = __builtin_amdgcn_readfirstlane((uint32_t)p.io.phase[phi]);
            // ---- IterativelyCalcS: from layer m, where the block of phase phi starts, down to
            // the single LLR of layer n
            int m = 0, local = 0;
            if (phi) {
                m = n - 1 - __builtin_ctz((unsigned)phi);
                local = 1;
            }
            for (int j = m; j < n; ++j) {
                const int loc = (j == m) ? local : 0;
                const int lgd = n - 1 - j;  // d = U >> (j + 1)
                const int d = 1 << lgd;
                if (lgd >= 2) {  // four LLRs to a lane
                    const int lgw = lgd - 2, dw = 1 << lgw;
                    const int tot = nact << lgw;
                    for (int it = lane; it < tot; it += 64) {
                        const int q = (int)act[it >> lgw], w = it & (dw - 1), s = 4 * w;
                        int8_t *sq = S + (size_t)q * pathS;
                        uint32_t a, b;
                        if (j == 0) {
                            a = chan4(s);
                            b = chan4(d + s);
                        } else {
                            const uint32_t *src = reinterpret_cast<const uint32_t *>(sq + s_off(U, j));
                            a = src[w];
                            b = src[dw + w];
                        }
                        uint32_t r;
                        if (loc) {
                            const uint32_t u4 = (C[(size_t)q * pathC + p.cwoff[j + 1] + (s >> 5)] >> (s & 31)) & 15u;
                            r = q8_g4(a, b, u4);
                        } else {
                            r = q8_f4(a, b);
                        }
                        reinterpret_cast<uint32_t *>(sq + s_off(U, j + 1))[w] = r;
                    }
                } else {
                    const int tot = nact << lgd;
                    for (int it = lane; it < tot; it += 64) {
                        const int q = (int)act[it >> lgd], s = it & (d - 1);
                        int8_t *sq = S + (size_t)q * pathS;
                        int a, b;
                        if (j == 0) {
                            a = chan(s);
                            b = chan(d + s);
                        } else {
                            const int8_t *src = sq + s_off(U, j);
                            a = src[s];
                            b = src[d + s];
                        }
                        int r;
                        if (loc) {
                            const uint32_t u = (C[(size_t)q * pathC + p.cwoff[j + 1] + (s >> 5)] >> (s & 31)) & 1u;
                            r = q8_g(a, b, u);
                        } else {
                            r = q8_f(a, b);
                        }
                        sq[s_off(U, j + 1) + s] = (int8_t)r;
                    }
                }
                wsync();
            }
            const bool on = mine && ((active >> lane) & 1u);
            if (on) pr.lv = (float)S[(size_t)lane * pathS + U - 2];
            const uint64_t corr = (e & kPhaseCorr) ? p.io.dfcorr[phi] : 0ull;
            uint32_t dec = 0;

            if (e & kPhaseFrozen) {
                dec = frozen_step(e, on, pr);
            } else {
                const Continuations ct = unfrozen_select(pr, active, nact, st, lane, L);
                dec = own_decision(ct.cont, pr.lv);
                // kills done; then the clones, in path order
                for (uint32_t cl = ct.clones; cl; cl &= cl - 1) {
                    const int l = __builtin_ctz(cl);
                    const int l1 = (int)st.pop(lane);  // ClonePath: copy the live state of l
                    {
                        // S_j (j >= 1) is read again iff bit n-1-j of phi is 0; copy from the
                        // first such layer on, in 16-byte pieces. The packed partial sums are
                        // copied whole.
                        const uint32_t zs = ~(uint32_t)phi & ((1u << (n - 1)) - 1u);
                        const int send = pathS - 16;
                        const int s0 = zs ? (s_off(U, n - 1 - (31 - __builtin_clz(zs))) & ~15) : send;
                        const int ns16 = (send - s0) >> 4;
                        const int nc = pathC;
                        const int nr = k >> 5;
                        const uint4 *sS = reinterpret_cast<const uint4 *>(S + (size_t)l * pathS + s0);
                        uint4 *dS = reinterpret_cast<uint4 *>(S + (size_t)l1 * pathS + s0);
                        const uint32_t *sC = C + (size_t)l * pathC;
                        uint32_t *dC = C + (size_t)l1 * pathC;
                        int top = ns16 > nc ? ns16 : nc;
                        top = top > nr ? top : nr;
                        for (int i = lane; i < top; i += 64) {
                            uint4 vs;
                            uint32_t vc = 0, vr = 0;
                            if (i < ns16) vs = sS[i];
                            if (i < nc) vc = sC[i];
                            if (i < nr) vr = rec[l * RW + i];
                            if (i < ns16) dS[i] = vs;
                            if (i < nc) dC[i] = vc;
                            if (i < nr) rec[l1 * RW + i] = vr;
                        }
                    }
                    clone_regs(pr, dec, l, l1, lane);
                    active |= 1u << l1;
                }
                wsync();
            }
            const bool now = mine && ((active >> lane) & 1u);
            if (now) {  // the path's own word: no other lane writes it
                uint32_t &w = C[(size_t)lane * pathC + lastc];
                const uint32_t bit = 1u << (phi & 1);
                w = dec ? (w | bit) : (w & ~bit);
                apply_correction(now, dec, corr, pr);
            }
            if (!(e & kPhaseFrozen)) {
                record_decision(now, dec, pr, k, rec, RW, lane);
                nact = list_active(active, act, lane, L);
            } else {
                wsync();
            }

            // ---- IterativelyUpdateC: the blocks this phase completes are encoded into their
            // parents' slots (the f32 kernel's butterflies)
            {
                int lam = n, lgs = 0, ph2 = phi;
                while (lam > 0 && (ph2 & 1)) {
                    const int psi = ph2 >> 1;
                    const int stride = 1 << lgs, next = stride << 1;
                    const int phi0 = (lam > 1) ? (psi & 1) * next : 0;
                    if (stride >= 32) {  // whole words: (x0, x1) -> (x0 ^ x1, x1), 32 at a time
                        const int lw = lgs - 5, sw = 1 << lw, tot = nact << lw;
                        for (int it = lane; it < tot; it += 64) {
                            const int q = (int)act[it >> lw], s = it & (sw - 1);
                            const uint32_t *src = C + (size_t)q * pathC + p.cwoff[lam];
                            uint32_t *dst = C + (size_t)q * pathC + p.cwoff[lam - 1] + (phi0 >> 5);
                            const uint32_t x0 = src[s], x1 = src[sw + s];
                            dst[s] = x0 ^ x1;
                            dst[sw + s] = x1;
                        }
                    } else if (mine && ((active >> lane) & 1u)) {  // one word per path, its lane
                        const uint32_t v = C[(size_t)lane * pathC + p.cwoff[lam]];
                        const uint32_t mk = (1u << stride) - 1u;
                        const uint32_t x0 = v & mk, x1 = (v >> stride) & mk;
                        const uint32_t r = (x0 ^ x1) | (x1 << stride);  // 2 stride bits
                        uint32_t &w = C[(size_t)lane * pathC + p.cwoff[lam - 1] + (phi0 >> 5)];
                        if (next == 32) {
                            w = r;
                        } else {
                            const int sh = phi0 & 31;
                            const uint32_t m2 = ((1u << next) - 1u) << sh;
                            w = (w & ~m2) | (r << sh);
                        }
                    }
                    wsync();
                    ++lgs;
                    ph2 = psi;
                    --lam;
                }
            }
        }
        const bool me = mine && ((active >> lane) & 1u);
        flush_record(pr, k, me, rec, RW, lane);

        // ---- final order: active paths by (R, index), descending; the f32 kernel's epilogue
        const int rk = rank_greater(pr.R, me, lane);
        for (int r = 0; r < nact; ++r) {
            const int q = (int)__builtin_ctzll(__ballot(me && rk == r));
            const uint32_t *cq = C + (size_t)q * pathC;  // C_0: the unshortened codeword (bits)
            const uint32_t *rq = rec + q * RW;
            const size_t row = (size_t)cw * L + r;
            if ((K & 3) == 0) {  // information bits, four per lane and store
                uint32_t *o4 = reinterpret_cast<uint32_t *>(p.io.info + row * K);
                for (int w = lane; w < (K >> 2); w += 64) {
                    const uint32_t bits = (rq[w >> 3] >> ((w & 7) * 4)) & 15u;
                    o4[w] = (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
                }
            } else {
                for (int kk = lane; kk < K; kk += 64) p.io.info[row * K + kk] = (uint8_t)((rq[kk >> 5] >> (kk & 31)) & 1u);
            }
            if (p.io.cw) {
                if ((p.N & 3) == 0) {
                    uint32_t *o4 = reinterpret_cast<uint32_t *>(p.io.cw + row * p.N);
                    for (int w = lane; w < (p.N >> 2); w += 64) {
                        const int i0 = 4 * w;
                        auto bitat = [&](int i) { return (cq[i >> 5] >> (i & 31)) & 1u; };
                        o4[w] = bitat(p.io.cwpos[i0]) | (bitat(p.io.cwpos[i0 + 1]) << 8) |
                                (bitat(p.io.cwpos[i0 + 2]) << 16) | (bitat(p.io.cwpos[i0 + 3]) << 24);
                    }
                } else {
                    for (int i = lane; i < p.N; i += 64) {
                        const int ci = p.io.cwpos[i];
                        p.io.cw[row * p.N + i] = (uint8_t)((cq[ci >> 5] >> (ci & 31)) & 1u);
                    }
                }
            }
            if (lane == 0) p.io.metric[row] = rdl_f(pr.R, q);
        }
        if (lane == 0) p.io.count[cw] = nact;
        wsync();
    }
}

// q = clamp(rint(llr * scale), -qmax, qmax): the product in f32, ties to even, NaN -> 0. Four
// elements per thread where the pointers allow whole 16-byte loads (vec), the tail one by one.
__device__ __forceinline__ int q8_quant(float x, float scale, float qmax) {
    const float v = rintf(x * scale);
    return v != v ? 0 : (int)fminf(fmaxf(v, -qmax), qmax);
}
template <bool VEC>
__global__ void __launch_bounds__(256) polar_quantize_kernel(const float *llr, size_t count, float scale, float qmax,
                                                             int8_t *q) {
    const size_t step = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t done = 0;
    if (VEC) {
        const size_t n4 = count >> 2;
        const float4 *l4 = reinterpret_cast<const float4 *>(llr);
        uint32_t *q4 = reinterpret_cast<uint32_t *>(q);
        for (size_t i = t0; i < n4; i += step) {
            const float4 v = l4[i];
            q4[i] = q8_put(q8_quant(v.x, scale, qmax), 0) | q8_put(q8_quant(v.y, scale, qmax), 1) |
                    q8_put(q8_quant(v.z, scale, qmax), 2) | q8_put(q8_quant(v.w, scale, qmax), 3);
        }
        done = n4 << 2;
    }
    for (size_t i = done + t0; i < count; i += step) q[i] = (int8_t)q8_quant(llr[i], scale, qmax);
}

hipError_t launch_polar_q8(const PolarQ8Params &p, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(polar_sclist_q8_kernel, dim3(grid), dim3(64), lds, s, p);
    return hipGetLastError();
}

const void *polar_q8_kernel_ptr() { return reinterpret_cast<const void *>(&polar_sclist_q8_kernel); }

hipError_t launch_polar_quantize(const float *llr, size_t count, float scale, int qmax, int8_t *q, hipStream_t s) {
    const bool vec = ((reinterpret_cast<uintptr_t>(llr) & 15u) | (reinterpret_cast<uintptr_t>(q) & 3u)) == 0;
    const size_t items = vec ? (count >> 2) + 3 : count;
    const unsigned grid = (unsigned)((items + 255) / 256 < 65536 ? (items + 255) / 256 : 65536);
    if (vec)
        hipLaunchKernelGGL(polar_quantize_kernel<true>, dim3(grid), dim3(256), 0, s, llr, count, scale, (float)qmax, q);
    else
        hipLaunchKernelGGL(polar_quantize_kernel<false>, dim3(grid), dim3(256), 0, s, llr, count, scale, (float)qmax, q);
    return hipGetLastError();
}

}  // namespace bchk
