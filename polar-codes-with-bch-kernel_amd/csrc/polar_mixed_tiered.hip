// polar_mixed_tiered.hip -- polar_mixed_kernel (polar_mixed.hip) for codes whose list state
// does not fit LDS: the same SC-list decoder over mixed kernels (Arikan, matrix and named
// layers), with the outer layers of every path in global memory.
//
// Same decisions, same float arithmetic and same path indices as polar_mixed_kernel: the list
// bookkeeping is the one copy in polar_list_device.h and the LLR and partial-sum routines are
// those of polar_llr_device.h, called with accessors into either tier, so the lists are the LDS
// kernel's bit for bit. One 64-lane wave per codeword, persistent over the batch. Codes with an
// ordered-statistics layer are not taken (the host refuses them).
//
// Tiers (PolarMixedTieredParams / PolarMixedTieredLayout, polar_device.h): for a layer j < split
// its group -- S_{j+1}, a named layer's floats F_j, C_{j+1} and the offset state O_j -- lies in
// the workgroup's workspace, as do C_0 and the channel LLRs after LoadLLRs (the LLR routines
// take pointers, so the mapped row is written once per codeword, there and not into LDS); the
// layers j >= split stay in LDS in the mixed layout of the inner sub-code, copied eagerly by a
// clone as in polar_mixed_kernel.
//
// Global groups are shared between paths, not copied (Tal and Vardy's lazy copy, as in
// polar_sclist_tiered.hip): per group there are L arrays and idx[j][q] names the array of path
// q; a clone copies the indices, a kill does nothing. All active paths write group j at the
// same phases -- layer j's LLR step, and the partial sums that finish a block of layer j + 1
// (for the last layer: the decision itself) -- so sharing is resolved once per write
// (own_group): of the paths that name the same array one keeps it, the others take arrays no
// active path names. References are counted from the index table when needed, never stored.
// What a path that moves takes along, at local phase loc of layer j:
//   the LLR step at loc = 0: nothing (S_{j+1} is rewritten whole, O_j cleared, F_j rewritten,
//     and C_{j+1} is written from piece 0 before any of it is read);
//   the LLR step at loc > 0, and the partial sums that write piece loc of C_{j+1} (any loc): the
//     pieces [0, loc) of C_{j+1}, O_j whole (matrix_offsets updates it in place from phase to
//     phase; A5's bit is there) and F_j whole. Never S_{j+1}: the next LLR step rewrites it.
// Array indices only select memory: every order and tie-break is on path indices.
// `j < split` is wave-uniform and branched on, so each call of a routine sees one address space
// per argument: LDS accesses stay ds_*, workspace accesses global_* (none flat).
// Shared text: LoadLLRs (plist::chan_llr), SoftXOR (pllr::soft_xor) and the index table's
// tier_init / tier_clone (polar_tier_device.h); own_group is the twin of the other tiered kernel's
// routine, kept apart by the speed gate of DESIGN 5.17.
// No MFMA: float min/add and byte XOR on short vectors, plain vector loads and stores.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_list_device.h"
#include "polar_llr_device.h"
#include "polar_tier_device.h"

namespace bchk {

using namespace plist;

__global__ void __launch_bounds__(64) polar_mixed_tiered_kernel(PolarMixedTieredParams tp) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const PolarMixedParams &p = tp.m;
    const int lane = (int)threadIdx.x;
    const int U = p.U, nl = p.nl, L = p.L, K = p.K, sp = tp.split;
    const int RW = polar_rec_words(K);
    const PolarMixedTieredLayout lo =
        polar_mixed_tiered_layout(U, L, K, p.ssize, p.csize, p.osize, nl, sp, p.tstates, tp.grp_bytes);
    // LDS by byte offsets from smem (integer casts of the pointers would make the accesses FLAT)
    float *S = reinterpret_cast<float *>(smem);
    uint8_t *C = smem + lo.o_C;
    uint8_t *O = smem + lo.o_O;
    uint8_t *idx = smem + lo.o_idx;
    uint8_t *own = smem + lo.o_own;
    uint16_t *ph = reinterpret_cast<uint16_t *>(smem + lo.o_ph);
    uint64_t *rows = reinterpret_cast<uint64_t *>(smem + lo.o_rows);  // [layer][row] bitmasks
    uint32_t *act = reinterpret_cast<uint32_t *>(smem + lo.o_act);
    uint32_t *rec = act + L;
    float *tmet = reinterpret_cast<float *>(smem + lo.o_tm);  // trellis state metrics, 2 x tstates
    uint8_t *wsb = tp.ws + (size_t)blockIdx.x * lo.ws_bytes;
    float *chan = reinterpret_cast<float *>(wsb);
    uint8_t *C0 = wsb + lo.w_C0;
    uint8_t *G = wsb + lo.w_grp;
    const bool mine = lane < L;
    const uint32_t lmask = L >= 32 ? 0xFFFFFFFFu : (1u << L) - 1u;
    for (int i = lane; i < U; i += 64) ph[i] = p.io.phase[i];
    for (int i = lane; i < kPolarMaxKernel * nl; i += 64) rows[i] = p.krows[i];

    // the global tier: path q's array of group j, and its parts (S_0: the channel; C_0: the path's own)
    auto gA = [&](int q, int j) -> uint8_t * {
        return G + (size_t)tp.gbase[j] + (size_t)idx[j * L + q] * (size_t)tp.garr[j];
    };
    auto gS = [&](int q, int lam) -> float * { return lam == 0 ? chan : reinterpret_cast<float *>(gA(q, lam - 1)); };
    auto gC = [&](int q, int lam) -> uint8_t * { return lam == 0 ? C0 + (size_t)q * lo.c0 : gA(q, lam - 1) + p.coff[lam]; };
    auto gO = [&](int q, int j) -> uint8_t * { return gA(q, j) + p.ooff[j]; };
    auto gF = [&](int q, int j) -> float * { return reinterpret_cast<float *>(gA(q, j)) + p.foff[j]; };
    // the LDS tier (layers lam > split, j >= split)
    auto lS = [&](int q, int lam) -> float * { return S + (size_t)q * p.ssize + p.soff[lam]; };
    auto lC = [&](int q, int lam) -> uint8_t * { return C + (size_t)q * p.csize + p.coff[lam]; };
    auto lO = [&](int q, int j) -> uint8_t * { return O + (size_t)q * p.osize + p.ooff[j]; };
    auto lF = [&](int q, int j) -> float * { return S + (size_t)q * p.ssize + p.foff[j]; };
    auto pathof = [&](int k) -> int { return (int)act[k]; };  // the k-th active path
    const pllr::Trellis tr{p.tent, p.tbase, p.tlog, tmet, p.tstates};

    // Before the active paths (`on`: this lane's path is one) write group j: every one of them
    // gets an array of its own. A path that moves takes cbytes of C_{j+1} along and, with
    // `state`, O_j and F_j (see the head of the file). Copies run in 32-bit words: the parts of
    // an array start on 16 bytes, and what a rounded-up word adds is written again before it is read.
    auto own_group = [&](int j, int cbytes, bool state, bool on) {
        uint8_t *ix = idx + j * L;
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
        const int wc = (cbytes + 3) >> 2;
        const int wo = state ? (tp.gobytes[j] + 3) >> 2 : 0;
        const int wf = state ? tp.gfloats[j] : 0;
        if (wc + wo + wf) {
            uint8_t *g0 = G + (size_t)tp.gbase[j];
            const int oc = p.coff[j + 1], oo = p.ooff[j], of = 4 * p.foff[j];
            for (uint32_t mv = movers; mv; mv &= mv - 1) {
                const int l = __builtin_ctz(mv);
                const uint8_t *src = g0 + (size_t)rdl_u((uint32_t)a, l) * (size_t)tp.garr[j];
                uint8_t *dst = g0 + (size_t)rdl_u((uint32_t)na, l) * (size_t)tp.garr[j];
                for (int i = lane; i < wc; i += 64)
                    reinterpret_cast<uint32_t *>(dst + oc)[i] = reinterpret_cast<const uint32_t *>(src + oc)[i];
                for (int i = lane; i < wo; i += 64)
                    reinterpret_cast<uint32_t *>(dst + oo)[i] = reinterpret_cast<const uint32_t *>(src + oo)[i];
                for (int i = lane; i < wf; i += 64)
                    reinterpret_cast<uint32_t *>(dst + of)[i] = reinterpret_cast<const uint32_t *>(src + of)[i];
            }
        }
        wsync();
    };

    // layer j's LLR step at local phase loc (d elements per path, tot items) over one choice of
    // accessors: polar_mixed_kernel's dispatch, without the search
    auto llr_step = [&](int j, int loc, int d, int tot, auto Sof, auto Cof, auto Oof, auto Fof) {
        const int l = p.ksize[j];
        if (p.arikan[j]) {
            pllr::arikan_llrs(j, loc, d, tot, lane, pathof, Sof, Cof);
            wsync();
            return;
        }
        if (p.named[j]) {  // G / A5: the f/g processor over the path's carried state
            pllr::named_llrs(p.named[j], j, loc, d, tot, lane, pathof, Sof, Cof, Fof, Oof);
            wsync();
            return;
        }
        // matrix layer: offset state, then the min-sum LLR per element
        const uint64_t *kr = rows + kPolarMaxKernel * j;
        pllr::matrix_offsets(kr, j, l, loc, d, tot, lane, pathof, Cof, Oof);
        wsync();
        if (p.trellis[j]) {
            pllr::trellis_llrs(tr, j, l, loc, d, tot, lane, pathof, Sof, Oof);
            return;
        }
        pllr::enum_llrs(kr, j, l, loc, d, tot, lane, pathof, Sof, Oof);
        wsync();
    };

    const int lastsz = p.ksize[nl - 1];
    PathStack st;
    st.slot = 0;
    wsync();
    for (uint32_t cw = blockIdx.x; cw < p.B; cw += gridDim.x) {
        // ---- LoadLLRs (MixedKernelEncoder.cpp:181-207), from the caller's row into the workspace
        const float *y = p.io.llr + (size_t)cw * p.N;
        for (int i = lane; i < U; i += 64) chan[i] = chan_llr(p.io.symmap, y, i);
        // the initial path names array 0 of every group, whatever the last codeword left
        st.reset(L, lane);
        const uint32_t pid = st.pop(lane);
        uint32_t active = 1u << pid;
        PathRegs pr{0.0f, 0.0f, 0ull, 0u};
        int k = 0;
        ptier::tier_init(idx, sp, L, pid, lane);
        wsync();
        int nact = list_active(active, act, lane, L);
        for (int phi = 0; phi < U; ++phi) {
            const uint32_t e = __builtin_amdgcn_readfirstlane((uint32_t)ph[phi]);
            const bool on = mine && ((active >> lane) & 1u);
            // ---- IterativelyCalcS (KernelListEngine.cpp:370-447)
            int m = nl - 1;
            uint32_t pq = (uint32_t)phi;
            while (m > 0 && pq % (uint32_t)p.ksize[m] == 0) {
                pq /= (uint32_t)p.ksize[m];
                --m;
            }
            for (int j = m; j < nl; ++j) {
                const int loc = (j == m) ? (int)(pq % (uint32_t)p.ksize[j]) : 0;
                const int d = p.outer[j + 1];
                const int tot = nact * d;
                if (j < sp) {
                    own_group(j, loc * d, loc != 0, on);
                    llr_step(j, loc, d, tot, gS, gC, gO, gF);
                } else if (j == sp) {  // across the boundary: S_split from the workspace, the rest in LDS
                    llr_step(sp, loc, d, tot,
                             [&](int q, int lam) -> float * { return lam == sp ? gS(q, lam) : lS(q, lam); }, lC, lO, lF);
                } else {
                    llr_step(j, loc, d, tot, lS, lC, lO, lF);
                }
            }
            if (on) {  // (a load per tier: one load through a selected pointer would be FLAT)
                if (nl <= sp)
                    pr.lv = gS(lane, nl)[0];
                else
                    pr.lv = lS(lane, nl)[0];
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
                    // ... and copies its LDS state
                    for (int i = lane; i < p.ssize; i += 64) S[(size_t)l1 * p.ssize + i] = S[(size_t)l * p.ssize + i];
                    for (int i = lane; i < p.csize; i += 64) C[(size_t)l1 * p.csize + i] = C[(size_t)l * p.csize + i];
                    for (int i = lane; i < p.osize; i += 64) O[(size_t)l1 * p.osize + i] = O[(size_t)l * p.osize + i];
                    for (int i = lane; i < (k >> 5); i += 64) rec[l1 * RW + i] = rec[l * RW + i];
                    clone_regs(pr, dec, l, l1, lane);
                    active |= 1u << l1;
                }
                wsync();
            }
            const bool now = mine && ((active >> lane) & 1u);
            const int lp = phi % lastsz;  // the decision is piece lp of C_nl
            if (nl <= sp) own_group(nl - 1, lp, true, now);
            if (now) {
                if (nl <= sp)
                    gC(lane, nl)[lp] = (uint8_t)dec;
                else
                    lC(lane, nl)[lp] = (uint8_t)dec;
                apply_correction(now, dec, corr, pr);
            }
            if (!(e & kPhaseFrozen)) {
                record_decision(now, dec, pr, k, rec, RW, lane);
                nact = list_active(active, act, lane, L);
            } else {
                wsync();
            }
            // ---- IterativelyUpdateC (KernelListEngine.cpp:266-315), pllr::update_c's loop with
            // the tier of each layer: finished blocks are multiplied by their kernel into the
            // parent layer's inputs
            {
                int lam = nl, stride = 1;
                uint32_t ph2 = (uint32_t)phi;
                while (lam > 0 && (ph2 + 1) % (uint32_t)p.ksize[lam - 1] == 0) {
                    const int l = p.ksize[lam - 1];
                    const uint32_t psi = ph2 / (uint32_t)l;
                    const int next = stride * l;
                    const int pc = lam > 1 ? (int)(psi % (uint32_t)p.ksize[lam - 2]) : 0;  // the piece of C_{lam-1} written
                    const int phi0 = pc * next;
                    const uint64_t *kr = rows + kPolarMaxKernel * (lam - 1);
                    const int tl = lam - 1;
                    if (tl > sp) {
                        pllr::update_c_layer(kr, l, stride, phi0, nact, lane, pathof, [&](int q) { return lC(q, lam); },
                                             [&](int q) { return lC(q, tl); });
                    } else {
                        if (tl >= 1) own_group(tl - 1, phi0, true, now);
                        auto dst = [&](int q) { return gC(q, tl); };
                        if (lam > sp)
                            pllr::update_c_layer(kr, l, stride, phi0, nact, lane, pathof, [&](int q) { return lC(q, lam); }, dst);
                        else
                            pllr::update_c_layer(kr, l, stride, phi0, nact, lane, pathof, [&](int q) { return gC(q, lam); }, dst);
                    }
                    wsync();
                    stride = next;
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
            const uint8_t *cq = C0 + (size_t)q * lo.c0;  // C_0: the unshortened codeword
            const uint32_t *rq = rec + q * RW;
            const size_t row = (size_t)cw * L + r;
            for (int kk = lane; kk < K; kk += 64) p.io.info[row * K + kk] = (uint8_t)((rq[kk >> 5] >> (kk & 31)) & 1u);
            if (p.io.cw)
                for (int i = lane; i < p.N; i += 64) p.io.cw[row * p.N + i] = cq[p.io.cwpos[i]];
            if (lane == 0) p.io.metric[row] = rdl_f(pr.R, q);
        }
        if (lane == 0) p.io.count[cw] = nact;
        wsync();
    }
}

hipError_t launch_polar_mixed_tiered(const PolarMixedTieredParams &p, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(polar_mixed_tiered_kernel, dim3(grid), dim3(64), lds, s, p);
    return hipGetLastError();
}

const void *polar_mixed_tiered_kernel_ptr() { return reinterpret_cast<const void *>(&polar_mixed_tiered_kernel); }

}  // namespace bchk
