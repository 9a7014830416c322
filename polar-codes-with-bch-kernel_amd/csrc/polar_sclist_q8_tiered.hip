// polar_sclist_q8_tiered.hip -- fixed-point SC-list decoding of all-Arikan polar codes whose
// int8 list state does not fit LDS: the arithmetic of polar_sclist_q8.hip in the tiers of
// polar_sclist_tiered.hip.
//
// Arithmetic and load rule are the int8 contract of include/bchk.h and DESIGN 5.18, restated in
// tests/sclist_q8.py:
//   load   -128 reads as -127, a punctured symbol is 0, a shortened one +127
//   f      sgn(a) sgn(b) min(|a|, |b|)
//   g      clamp(u ? b - a : b + a, -127, +127)
//   metric a decision against the sign of v costs |v|
// so the lists are polar_sclist_q8_kernel's bit for bit wherever both take the code. Metrics and
// the leaf LLR are floats (exact integers below 2^24) and the list bookkeeping is plist::
// (polar_list_device.h), called unchanged.
//
// State handling is the f32 tiered kernel's (polar_q8_tiered_layout, polar_device.h): S_λ and C_λ
// with λ <= split, and C_0, lie in the workgroup's workspace in global memory, shared between
// paths through idx and copied on write (own_layer; tier_init / tier_clone of
// polar_tier_device.h); the layers below the split stay in LDS, where a clone copies their live
// part in 16-byte pieces. A global S array holds U >> λ bytes; the packed C arrays are the f32
// tiered kernel's. What a mover takes along is what it takes there: nothing of S, and the first
// half of C where that half is live. The barrier and fence between the lanes' workspace writes
// and reads (plist::wsync) is unchanged: byte stores of different lanes into one dword are
// separate writes like any others.
//
// A layer of d >= 4 LLRs goes four to a lane on either side of the split: one 32-bit word per
// operand, one word stored, the four known bits of a g step from one extract of the packed C
// word. Layers of one or two LLRs go element by element with byte loads and stores. Layer 0 is
// gathered from the caller's int8 row through the LoadLLRs map. The f/g bodies, the butterflies
// and the epilogue are restated here as in every list kernel. No MFMA, no inline
// assembly.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_list_device.h"
#include "polar_tier_device.h"

namespace bchk {

namespace {

using namespace plist;

__device__ __forceinline__ int q8t_clamp(int v) { return v > kQ8Max ? kQ8Max : (v < -kQ8Max ? -kQ8Max : v); }
// LoadLLRs on int8 rows
__device__ __forceinline__ int q8t_chan(const int16_t *symmap, const int8_t *y, int i) {
    const int m = symmap[i];
    return m >= 0 ? q8t_clamp((int)y[m]) : (m == -1 ? kQ8Max : 0);
}
__device__ __forceinline__ int q8t_f(int a, int b) {
    const int ma = a < 0 ? -a : a, mb = b < 0 ? -b : b;
    const int m = ma < mb ? ma : mb;
    return ((a ^ b) < 0) ? -m : m;
}
__device__ __forceinline__ int q8t_g(int a, int b, uint32_t u) { return q8t_clamp(u ? b - a : b + a); }
// byte k of a packed word, sign-extended, and back
__device__ __forceinline__ int q8t_at(uint32_t w, int k) { return (int)(int8_t)(uint8_t)(w >> (8 * k)); }
__device__ __forceinline__ uint32_t q8t_put(int v, int k) { return ((uint32_t)v & 255u) << (8 * k); }
__device__ __forceinline__ uint32_t q8t_f4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= q8t_put(q8t_f(q8t_at(a, k), q8t_at(b, k)), k);
    return r;
}
__device__ __forceinline__ uint32_t q8t_g4(uint32_t a, uint32_t b, uint32_t u4) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= q8t_put(q8t_g(q8t_at(a, k), q8t_at(b, k), (u4 >> k) & 1u), k);
    return r;
}

}  // namespace

__global__ void __launch_bounds__(64) polar_sclist_q8_tiered_kernel(PolarQ8TieredParams qp) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const PolarTieredParams &tp = qp.t;
    const PolarParams &p = tp.p;
    const int lane = (int)threadIdx.x;
    const int U = p.U, n = p.n, L = p.L, K = p.K, sp = tp.split;
    const int Us = U >> sp, RW = polar_rec_words(K), cwsplit = tp.cwsplit;
    const PolarTieredLayout lo = polar_q8_tiered_layout(U, L, K, sp, cwsplit, tp.cwall);
    const int pathS = lo.pathS, pathC = lo.pathC;  // bytes, words
    // LDS by byte offsets from smem (integer casts of the pointers would make the accesses FLAT)
    int8_t *S = reinterpret_cast<int8_t *>(smem);
    uint32_t *C = reinterpret_cast<uint32_t *>(smem + lo.o_C);
    uint8_t *idx = smem + lo.o_idx;
    uint8_t *own = smem + lo.o_own;
    uint32_t *act = reinterpret_cast<uint32_t *>(smem + lo.o_act);
    uint32_t *rec = act + L;
    uint8_t *wsb = tp.ws + (size_t)blockIdx.x * lo.ws_bytes;
    int8_t *Sg = reinterpret_cast<int8_t *>(wsb);
    uint32_t *Cg = reinterpret_cast<uint32_t *>(wsb + lo.w_C);
    const bool mine = lane < L;
    const uint32_t lmask = L >= 32 ? 0xFFFFFFFFu : (1u << L) - 1u;

    // layer λ of array a (global tier, 1 <= λ <= split; C_0: a = the path) / of path q (LDS tier)
    auto gS = [&](int lam, int a) -> int8_t * { return Sg + (size_t)L * (U - (U >> (lam - 1))) + (size_t)a * (U >> lam); };
    auto gC = [&](int lam, int a) -> uint32_t * {
        return Cg + (size_t)L * p.cwoff[lam] + (size_t)a * polar_cw_words(U, lam);
    };
    auto lS = [&](int lam, int q) -> int8_t * { return S + (size_t)q * pathS + (Us - (U >> (lam - 1))); };
    auto lC = [&](int lam, int q) -> uint32_t * { return C + (size_t)q * pathC + (p.cwoff[lam] - cwsplit); };
    auto arr = [&](int lam, int q) -> int { return (int)idx[(lam - 1) * L + q]; };

    // Before the active paths (`on`: this lane's path is one) write global layer lam: every one
    // of them gets an array of its own. keep_x0: the first half of C_lam stays live (a sub-word
    // layer keeps its one word). The f32 tiered kernel's routine: it moves packed C only.
    auto own_layer = [&](int lam, bool keep_x0, bool on) {
        uint8_t *ix = idx + (lam - 1) * L;
        const int a = on ? (int)ix[lane] : 0;
        if (mine) own[lane] = 0xFF;
        wsync();
        if (on) own[a] = (uint8_t)lane;  // one of the paths naming a stays
        wsync();
        const uint32_t used = (uint32_t)__ballot(mine && own[lane] != 0xFF);
        const bool move = on && own[a] != (uint8_t)lane;
        const uint32_t movers = (uint32_t)__ballot(move);
        if (!movers) return;
        int na = 0;
        if (move) {  // the r-th mover takes the r-th array nobody names
            uint32_t fr = ~used & lmask;
            for (int r = __builtin_popcount(movers & ((1u << lane) - 1u)); r > 0; --r) fr &= fr - 1;
            na = __builtin_ctz(fr);
            ix[lane] = (uint8_t)na;
        }
        if (keep_x0) {
            const int d = U >> lam;
            if (d <= 32) {
                if (move) gC(lam, na)[0] = gC(lam, a)[0];
            } else {
                const int w = d >> 5;
                for (uint32_t mv = movers; mv; mv &= mv - 1) {
                    const int l = __builtin_ctz(mv);
                    const uint32_t *src = gC(lam, (int)rdl_u((uint32_t)a, l));
                    uint32_t *dst = gC(lam, (int)rdl_u((uint32_t)na, l));
                    for (int i = lane; i < w; i += 64) dst[i] = src[i];
                }
            }
        }
        wsync();
    };

    // One layer of the LLR recursion: S_{j+1} = f or g of the two halves of S_j. ld4(q, w): word w
    // (four LLRs) of path q's S_j, ld1(q, i): its LLR i; dst(q): S_{j+1}, cw(q): C_{j+1}.
    auto fg_layer = [&](int j, int loc, int nact, auto ld4, auto ld1, auto dst, auto cw) {
        const int lgd = n - 1 - j;  // d = U >> (j + 1)
        const int d = 1 << lgd;
        if (lgd >= 2) {  // four LLRs to a lane
            const int lgw = lgd - 2, dw = 1 << lgw;
            const int tot = nact << lgw;
            for (int it = lane; it < tot; it += 64) {
                const int q = (int)act[it >> lgw], w = it & (dw - 1), s = 4 * w;
                const uint32_t a = ld4(q, w), b = ld4(q, dw + w);
                uint32_t r;
                if (loc) {  // s is a multiple of 4: the four bits never straddle a word
                    const uint32_t u4 = (cw(q)[s >> 5] >> (s & 31)) & 15u;
                    r = q8t_g4(a, b, u4);
                } else {
                    r = q8t_f4(a, b);
                }
                reinterpret_cast<uint32_t *>(dst(q))[w] = r;
            }
        } else {
            const int tot = nact << lgd;
            for (int it = lane; it < tot; it += 64) {
                const int q = (int)act[it >> lgd], s = it & (d - 1);
                const int a = ld1(q, s), b = ld1(q, d + s);
                int r;
                if (loc) {
                    const uint32_t u = (cw(q)[s >> 5] >> (s & 31)) & 1u;
                    r = q8t_g(a, b, u);
                } else {
                    r = q8t_f(a, b);
                }
                dst(q)[s] = (int8_t)r;
            }
        }
    };

    // the Arikan kernel's output of a finished block: C_lam (x0, x1) -> (x0 ^ x1, x1) at bit phi0
    // of C_{lam-1}; stride = bits of x0
    auto butterfly = [&](int lgs, int phi0, int nact, bool on, auto srcw, auto dstw) {
        const int stride = 1 << lgs, next = stride << 1;
        if (stride >= 32) {  // whole words, 32 at a time
            const int lw = lgs - 5, sw = 1 << lw, tot = nact << lw;
            for (int it = lane; it < tot; it += 64) {
                const int q = (int)act[it >> lw], s = it & (sw - 1);
                const uint32_t *src = srcw(q);
                uint32_t *dst = dstw(q) + (phi0 >> 5);
                const uint32_t x0 = src[s], x1 = src[sw + s];
                dst[s] = x0 ^ x1;
                dst[sw + s] = x1;
            }
        } else if (on) {  // one word per path, its lane
            const uint32_t v = srcw(lane)[0];
            const uint32_t mk = (1u << stride) - 1u;
            const uint32_t x0 = v & mk, x1 = (v >> stride) & mk;
            const uint32_t r = (x0 ^ x1) | (x1 << stride);  // 2 stride bits
            uint32_t &w = dstw(lane)[phi0 >> 5];
            if (next == 32) {
                w = r;
            } else {
                const int sh = phi0 & 31;
                const uint32_t m2 = ((1u << next) - 1u) << sh;
                w = (w & ~m2) | (r << sh);
            }
        }
    };

    PathStack st;
    st.slot = 0;
    for (uint32_t cw = blockIdx.x; cw < p.B; cw += gridDim.x) {
        // ---- LoadLLRs, applied where layer 0 is read
        const int8_t *y = qp.llr8 + (size_t)cw * p.N;
        auto chan = [&](int i) -> int { return q8t_chan(p.io.symmap, y, i); };
        auto chan4 = [&](int i) -> uint32_t {
            return q8t_put(chan(i), 0) | q8t_put(chan(i + 1), 1) | q8t_put(chan(i + 2), 2) | q8t_put(chan(i + 3), 3);
        };
        // ---- Cleanup + AssignInitialPath; the initial path names array 0 of every global
        // layer, whatever the last codeword left
        st.reset(L, lane);
        const uint32_t pid = st.pop(lane);
        uint32_t active = 1u << pid;
        PathRegs pr{0.0f, 0.0f, 0ull, 0u};
        int k = 0;  // unfrozen decisions so far
        ptier::tier_init(idx, sp, L, pid, lane);
        wsync();
        int nact = list_active(active, act, lane, L);

        for (int phi = 0; phi < U; ++phi) {
            const uint32_t e = __builtin_amdgcn_readfirstlane((uint32_t)p.io.phase[phi]);
            const bool on = mine && ((active >> lane) & 1u);
            // ---- IterativelyCalcS: from layer m, where the block of phase phi starts, down to
            // the single LLR of layer n
            int m = 0, local = 0;
            if (phi) {
                m = n - 1 - __builtin_ctz((unsigned)phi);
                local = 1;
            }
            for (int j = m; j < n; ++j) {
                const int loc = (j == m) ? local : 0;
                const int lam = j + 1;
                auto g4 = [&](int q, int w) { return reinterpret_cast<const uint32_t *>(gS(j, arr(j, q)))[w]; };
                auto g1 = [&](int q, int i) { return (int)gS(j, arr(j, q))[i]; };
                if (lam <= sp) {
                    own_layer(lam, loc != 0, on);
                    auto dst = [&](int q) { return gS(lam, arr(lam, q)); };
                    auto cwd = [&](int q) { return gC(lam, arr(lam, q)); };
                    if (j == 0)
                        fg_layer(j, loc, nact, [&](int, int w) { return chan4(4 * w); }, [&](int, int i) { return chan(i); },
                                 dst, cwd);
                    else
                        fg_layer(j, loc, nact, g4, g1, dst, cwd);
                } else {
                    auto dst = [&](int q) { return lS(lam, q); };
                    auto cwd = [&](int q) { return lC(lam, q); };
                    if (j == sp)
                        fg_layer(j, loc, nact, g4, g1, dst, cwd);
                    else
                        fg_layer(
                            j, loc, nact, [&](int q, int w) { return reinterpret_cast<const uint32_t *>(lS(j, q))[w]; },
                            [&](int q, int i) { return (int)lS(j, q)[i]; }, dst, cwd);
                }
                wsync();
            }
            if (on) {
                if (n <= sp)
                    pr.lv = (float)gS(n, arr(n, lane))[0];
                else
                    pr.lv = (float)lS(n, lane)[0];
            }
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
                    const int l1 = (int)st.pop(lane);  // ClonePath: l1 names l's global arrays ...
                    ptier::tier_clone(idx, sp, L, l, l1, lane);
                    {
                        // ... and copies the live state of l in LDS: S_j (j > split) is read
                        // again iff bit n-1-j of phi is 0; from the first such layer's offset,
                        // rounded down to 16, in 16-byte pieces. The packed partial sums whole;
                        // the record words.
                        const int lb = n - 1 - sp;  // layers split+1 .. n-1 <-> bits lb-1 .. 0
                        const uint32_t zs = lb > 0 ? (~(uint32_t)phi & ((1u << lb) - 1u)) : 0u;
                        const int send = pathS ? pathS - 16 : 0;
                        const int s0 = zs ? ((Us - (U >> (n - 2 - (31 - __builtin_clz(zs))))) & ~15) : send;
                        const int ns16 = (send - s0) >> 4;
                        const int nc = lo.n_C;
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
            if (n <= sp) own_layer(n, (phi & 1) != 0, now);
            if (now) {  // the path's own word: no other lane writes it
                const uint32_t bit = 1u << (phi & 1);
                auto put = [&](uint32_t &w) { w = dec ? (w | bit) : (w & ~bit); };
                if (n <= sp)
                    put(gC(n, arr(n, lane))[0]);
                else
                    put(lC(n, lane)[0]);
                apply_correction(now, dec, corr, pr);
            }
            if (!(e & kPhaseFrozen)) {
                record_decision(now, dec, pr, k, rec, RW, lane);
                nact = list_active(active, act, lane, L);
            } else {
                wsync();
            }

            // ---- IterativelyUpdateC: the blocks this phase completes are encoded into their
            // parents' slots
            {
                int lam = n, lgs = 0, ph2 = phi;
                while (lam > 0 && (ph2 & 1)) {
                    const int psi = ph2 >> 1;
                    const int phi0 = (lam > 1) ? (psi & 1) << (lgs + 1) : 0;
                    const int tl = lam - 1;  // the layer written: its half psi & 1
                    if (tl > sp) {
                        butterfly(lgs, phi0, nact, now, [&](int q) { return lC(lam, q); }, [&](int q) { return lC(tl, q); });
                    } else {
                        if (tl >= 1) own_layer(tl, (psi & 1) != 0, now);
                        auto dst = [&](int q) { return gC(tl, tl ? arr(tl, q) : q); };
                        if (lam > sp)
                            butterfly(lgs, phi0, nact, now, [&](int q) { return lC(lam, q); }, dst);
                        else
                            butterfly(lgs, phi0, nact, now, [&](int q) { return gC(lam, arr(lam, q)); }, dst);
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

        // ---- final order: active paths by (R, index), descending
        const int rk = rank_greater(pr.R, me, lane);
        for (int r = 0; r < nact; ++r) {
            const int q = (int)__builtin_ctzll(__ballot(me && rk == r));
            const uint32_t *cq = gC(0, q);  // C_0: the unshortened codeword (bits)
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

hipError_t launch_polar_q8_tiered(const PolarQ8TieredParams &p, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(polar_sclist_q8_tiered_kernel, dim3(grid), dim3(64), lds, s, p);
    return hipGetLastError();
}

const void *polar_q8_tiered_kernel_ptr() { return reinterpret_cast<const void *>(&polar_sclist_q8_tiered_kernel); }

}  // namespace bchk
