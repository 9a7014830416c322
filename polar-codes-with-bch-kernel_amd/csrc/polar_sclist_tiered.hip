// polar_sclist_tiered.hip -- polar_sclist_kernel (polar_sclist.hip) for codes whose list state
// does not fit LDS: the same SC-list decoder over the Arikan kernel, with the big layers of
// every path in global memory.
//
// Same decisions, same float arithmetic and same path indices as polar_sclist_kernel (the list
// bookkeeping is the one copy in polar_list_device.h), so the lists are the LDS kernel's bit for
// bit. One 64-lane wave per codeword, persistent over the batch.
//
// Tiers (PolarTieredLayout, polar_device.h): S_λ and C_λ with λ <= split, and C_0, lie in the
// workgroup's workspace in global memory; the layers below the split stay in LDS as in
// polar_sclist_kernel (a clone copies their live part eagerly).
//
// Global layers are shared between paths, not copied (Tal and Vardy's lazy copy; the
// reference's CTVMemoryEngine / CListKernelEngine::UpdateIndex, TVMemoryEngine.cpp:96-142,
// KernelListEngine.cpp:318-367). Per global layer there are L arrays, holding S_λ and C_λ
// together, and idx[λ][q] names the array of path q; a clone copies the indices. All active
// paths write a layer at the same phases, so sharing is resolved once per write (own_layer):
// of the paths that name the same array one keeps it, the others take arrays no active path
// names. An array's reference count is thus the number of active paths naming it, counted when
// it is needed and never stored: nothing to release at a kill, nothing to carry from one
// codeword to the next but the initial path's indices. What a path that moves takes along:
// nothing of S (f / g rewrite the whole layer), and of C the first half when the second is the
// one being written (or about to be read by g); the other cases leave nothing live. Array
// indices only select memory: every order and tie-break is on path indices.
// Shared text: LoadLLRs (plist::chan_llr), SoftXOR (pllr::soft_xor) and the index table's
// tier_init / tier_clone (polar_tier_device.h); own_layer is the twin of the other tiered kernel's
// routine, kept apart by the speed gate of DESIGN 5.17.
// No MFMA: float min/add and word XOR on short vectors, plain vector loads and stores.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_list_device.h"
#include "polar_llr_device.h"
#include "polar_tier_device.h"

namespace bchk {

namespace {

using namespace plist;

}  // namespace

__global__ void __launch_bounds__(64) polar_sclist_tiered_kernel(PolarTieredParams tp) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const PolarParams &p = tp.p;
    const int lane = (int)threadIdx.x;
    const int U = p.U, n = p.n, L = p.L, K = p.K, sp = tp.split;
    const int Us = U >> sp, RW = polar_rec_words(K), cwsplit = tp.cwsplit;
    const PolarTieredLayout lo = polar_tiered_layout(U, L, K, sp, cwsplit, tp.cwall);
    const int pathS = lo.pathS, pathC = lo.pathC;
    // LDS by byte offsets from smem (integer casts of the pointers would make the accesses FLAT)
    float *S = reinterpret_cast<float *>(smem);
    uint32_t *C = reinterpret_cast<uint32_t *>(smem + lo.o_C);
    uint8_t *idx = smem + lo.o_idx;
    uint8_t *own = smem + lo.o_own;
    uint32_t *act = reinterpret_cast<uint32_t *>(smem + lo.o_act);
    uint32_t *rec = act + L;
    uint8_t *wsb = tp.ws + (size_t)blockIdx.x * lo.ws_bytes;
    float *Sg = reinterpret_cast<float *>(wsb);
    uint32_t *Cg = reinterpret_cast<uint32_t *>(wsb + lo.w_C);
    const bool mine = lane < L;
    const uint32_t lmask = L >= 32 ? 0xFFFFFFFFu : (1u << L) - 1u;

    // layer λ of array a (global tier, 1 <= λ <= split; C_0: a = the path) / of path q (LDS tier)
    auto gS = [&](int lam, int a) -> float * { return Sg + (size_t)L * (U - (U >> (lam - 1))) + (size_t)a * (U >> lam); };
    auto gC = [&](int lam, int a) -> uint32_t * {
        return Cg + (size_t)L * p.cwoff[lam] + (size_t)a * polar_cw_words(U, lam);
    };
    auto lS = [&](int lam, int q) -> float * { return S + (size_t)q * pathS + (Us - (U >> (lam - 1))); };
    auto lC = [&](int lam, int q) -> uint32_t * { return C + (size_t)q * pathC + (p.cwoff[lam] - cwsplit); };
    auto arr = [&](int lam, int q) -> int { return (int)idx[(lam - 1) * L + q]; };

    // Before the active paths (`on`: this lane's path is one) write global layer lam: every one
    // of them gets an array of its own. keep_x0: the first half of C_lam stays live (a sub-word
    // layer keeps its one word).
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

    // one layer of the LLR recursion: S_{j+1} = f or g of the two halves of S_j
    auto fg_layer = [&](int j, int loc, int nact, auto src, auto dst, auto cw) {
        const int lgd = n - 1 - j;  // d = U >> (j + 1)
        const int d = 1 << lgd;
        const int tot = nact << lgd;
        for (int it = lane; it < tot; it += 64) {
            const int q = (int)act[it >> lgd], s = it & (d - 1);
            const float a = src(q, s), b = src(q, d + s);
            float r;
            if (loc) {  // SoftCombine (:39-50): b - a if u = 1 else b + a
                r = ((cw(q)[s >> 5] >> (s & 31)) & 1u) ? b - a : b + a;
            } else {
                r = pllr::soft_xor(a, b);
            }
            dst(q)[s] = r;
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
        // ---- LoadLLRs (MixedKernelEncoder.cpp:181-207), applied where layer 0 is read
        const float *y = p.io.llr + (size_t)cw * p.N;
        auto chan = [&](int i) -> float { return chan_llr(p.io.symmap, y, i); };
        // ---- Cleanup + AssignInitialPath (TVMemoryEngine.cpp:58-94); the initial path names
        // array 0 of every global layer, whatever the last codeword left
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
            // ---- IterativelyCalcS (KernelListEngine.cpp:370-447): from layer m, where the
            // block of phase phi starts, down to the single LLR of layer n
            int m = 0, local = 0;
            if (phi) {
                m = n - 1 - __builtin_ctz((unsigned)phi);
                local = 1;
            }
            for (int j = m; j < n; ++j) {
                const int loc = (j == m) ? local : 0;
                const int lam = j + 1;
                if (lam <= sp) {
                    own_layer(lam, loc != 0, on);
                    auto dst = [&](int q) { return gS(lam, arr(lam, q)); };
                    auto cwd = [&](int q) { return gC(lam, arr(lam, q)); };
                    if (j == 0)
                        fg_layer(j, loc, nact, [&](int, int i) { return chan(i); }, dst, cwd);
                    else
                        fg_layer(j, loc, nact, [&](int q, int i) { return gS(j, arr(j, q))[i]; }, dst, cwd);
                } else {
                    auto dst = [&](int q) { return lS(lam, q); };
                    auto cwd = [&](int q) { return lC(lam, q); };
                    if (j == sp)
                        fg_layer(j, loc, nact, [&](int q, int i) { return gS(j, arr(j, q))[i]; }, dst, cwd);
                    else
                        fg_layer(j, loc, nact, [&](int q, int i) { return lS(j, q)[i]; }, dst, cwd);
                }
                wsync();
            }
            if (on) {
                if (n <= sp)
                    pr.lv = gS(n, arr(n, lane))[0];
                else
                    pr.lv = lS(n, lane)[0];
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
                        // again iff bit n-1-j of phi is 0, from the first such layer on; the
                        // packed partial sums whole; the record words
                        const int lb = n - 1 - sp;  // layers split+1 .. n-1 <-> bits lb-1 .. 0
                        const uint32_t zs = lb > 0 ? (~(uint32_t)phi & ((1u << lb) - 1u)) : 0u;
                        const int top4 = (Us + 3) & ~3;
                        const int s0 = zs ? ((Us - (U >> (n - 2 - (31 - __builtin_clz(zs))))) & ~3) : top4;
                        const int ns4 = pathS ? (top4 - s0) >> 2 : 0;
                        const int nc = lo.n_C;
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

            // ---- IterativelyUpdateC (KernelListEngine.cpp:266-315): the blocks this phase
            // completes are encoded into their parents' slots
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

        // ---- final order (:249-267): active paths by (R, index), descending
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

hipError_t launch_polar_tiered(const PolarTieredParams &p, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(polar_sclist_tiered_kernel, dim3(grid), dim3(64), lds, s, p);
    return hipGetLastError();
}

const void *polar_tiered_kernel_ptr() { return reinterpret_cast<const void *>(&polar_sclist_tiered_kernel); }

}  // namespace bchk
