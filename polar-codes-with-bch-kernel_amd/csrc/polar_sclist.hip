// polar_sclist.hip -- batched SC-list decoding of polar codes over the Arikan kernel (with
// dynamic frozen constraints, shortening and puncturing) on gfx950.
//
// Reference: the vendored CMixedKernelListDecoder (out/external/MixedKernelListDecoder.cpp:
// 61-268) over CListKernelEngine (out/external/KernelListEngine.cpp:266-447), the f/g
// processor of headers/external/KernProc.h:89-102 (SoftProcessing.cpp:39-80) and the
// path-index stack of out/external/TVMemoryEngine.cpp:85-142. Same decisions, same float
// arithmetic and the same path indices (the list sorts break ties on them), so the output
// lists equal the CPU restatement (oracle/polar_oracle.c) bit for bit.
//
// Execution model: one 64-lane wave per codeword (persistent over the batch).
//   * LDS holds every path's LLRs S_λ (U >> λ floats) and partial sums C_λ (kernel inputs
//     of the current block, U >> (λ-1) bits packed in 32-bit words, each layer word-aligned;
//     C_0 = the codeword) and the information bits decided so far (packed, flushed every 32
//     decisions). The channel LLRs (read at two phases per codeword) and the phase table
//     come from global memory, so (1024, 512) at L = 8 fits 4 waves per CU.
//   * Lane q < L holds path q's scalar state in registers: metric R, leaf LLR, dynamic-
//     freezing mask, the current record word and slot q of the path-index stack (pushes and
//     pops are v_writelane / v_readlane on a wave-uniform top).
//   * Each phase: the LLR recursion from the first layer whose block changed, lanes over
//     (active path x element); decisions (frozen: lane = path; unfrozen: the 2 L candidates
//     ranked in lanes 2q + b with the reference's std::greater<pair> order); kills, then
//     clones in path order, a clone copying only the parent's live S layers, live C halves
//     and record words; then the partial-sum butterflies of the finished blocks.
// No MFMA: the work is float min/add and byte XOR on short vectors.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_list_device.h"
#include "polar_llr_device.h"

namespace bchk {

namespace {

using namespace plist;

// offset of S_λ (λ >= 1) inside one path's LLR array
__device__ __forceinline__ int s_off(int U, int lam) { return U - (U >> (lam - 1)); }

}  // namespace

__global__ void __launch_bounds__(64) polar_sclist_kernel(PolarParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = (int)threadIdx.x;
    const int U = p.U, n = p.n, L = p.L, K = p.K;
    const int pathS = polar_path_s(U), pathC = p.pathCw, RW = polar_rec_words(K);
    // LDS layout: polar_list_layout (polar_device.h)
    // (byte offsets from smem, never through integer casts of the pointers, which would
    // lose the LDS address space and turn every access into a FLAT one)
    const PolarListLayout lo = polar_list_layout(U, L, K, pathC);
    float *S = reinterpret_cast<float *>(smem);
    uint32_t *C = reinterpret_cast<uint32_t *>(smem + lo.o_C);  // packed bits, words per path
    uint32_t *act = reinterpret_cast<uint32_t *>(smem + lo.o_act);
    uint32_t *rec = act + L;
    const int lastc = p.cwoff[n];  // C_n: the two inputs of the last Arikan block (one word)
    const bool mine = lane < L;
    auto cbit = [&](int q, int lam, int s) -> uint32_t {
        const int b = s;
        return (C[(size_t)q * pathC + p.cwoff[lam] + (b >> 5)] >> (b & 31)) & 1u;
    };

    PathStack st;
    st.slot = 0;
    for (uint32_t cw = blockIdx.x; cw < p.B; cw += gridDim.x) {
        // ---- LoadLLRs (MixedKernelEncoder.cpp:181-207), applied where layer 0 is read
        const float *y = p.io.llr + (size_t)cw * p.N;
        auto chan = [&](int i) -> float { return chan_llr(p.io.symmap, y, i); };
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
            // ---- IterativelyCalcS (KernelListEngine.cpp:370-447): from layer m, where the
            // block of phase phi starts, down to the single LLR of layer n
            int m = 0, local = 0;
            if (phi) {
                m = n - 1 - __builtin_ctz((unsigned)phi);
                local = 1;
            }
            for (int j = m; j < n; ++j) {
                const int loc = (j == m) ? local : 0;
                const int lgd = n - 1 - j;  // d = U >> (j + 1)
                const int d = 1 << lgd;
                const int tot = nact << lgd;
                for (int it = lane; it < tot; it += 64) {
                    const int q = (int)act[it >> lgd], s = it & (d - 1);
                    float *dst = S + (size_t)q * pathS + s_off(U, j + 1);
                    float a, b;
                    if (j == 0) {
                        a = chan(s);
                        b = chan(d + s);
                    } else {
                        const float *src = S + (size_t)q * pathS + s_off(U, j);
                        a = src[s];
                        b = src[d + s];
                    }
                    float r;
                    if (loc) {  // SoftCombine (:39-50): b - a if u = 1 else b + a
                        r = cbit(q, j + 1, s) ? b - a : b + a;
                    } else {
                        r = pllr::soft_xor(a, b);
                    }
                    dst[s] = r;
                }
                wsync();
            }
            const bool on = mine && ((active >> lane) & 1u);
            if (on) pr.lv = S[(size_t)lane * pathS + U - 2];
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
                        // first such layer on. The packed partial sums are copied whole
                        // (3U bits).
                        const uint32_t zs = ~(uint32_t)phi & ((1u << (n - 1)) - 1u);
                        const int s0 = zs ? (s_off(U, n - 1 - (31 - __builtin_clz(zs))) & ~3) : pathS;
                        const int ns4 = (((U + 3) & ~3) - s0) >> 2;
                        const int nc = pathC;
                        const int nr = k >> 5;
                        const uint4 *sS = reinterpret_cast<const uint4 *>(S + (size_t)l * pathS + s0);
                        uint4 *dS = reinterpret_cast<uint4 *>(S + (size_t)l1 * pathS + s0);
                        const uint32_t *sC = C + (size_t)l * pathC;
                        uint32_t *dC = C + (size_t)l1 * pathC;
                        int top = ns4 > nc ? ns4 : nc;
                        top = top > nr ? top : nr;
                        for (int i = lane; i < top; i += 64) {
                            uint4 vs;
                            uint32_t vc = 0, vr = 0;
                            if (i < ns4) vs = sS[i];
                            if (i < nc) vc = sC[i];
                            if (i < nr) vr = rec[l * RW + i];
                            if (i < ns4) dS[i] = vs;
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

            // ---- IterativelyUpdateC (KernelListEngine.cpp:266-315): the blocks this phase
            // completes are encoded into their parents' slots
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

        // ---- final order (:249-267): active paths by (R, index), descending
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

hipError_t launch_polar(const PolarParams &p, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(polar_sclist_kernel, dim3(grid), dim3(64), lds, s, p);
    return hipGetLastError();
}

const void *polar_kernel_ptr() { return reinterpret_cast<const void *>(&polar_sclist_kernel); }

}  // namespace bchk
