// polar_list_device.h -- the list bookkeeping of SC-list decoding, shared by the all-Arikan
// kernels (polar_sclist.hip, polar_sclist_tiered.hip, and polar_sclist_q8.hip, whose int8 leaf LLRs
// and integer metrics are exact as floats) and the mixed-kernel ones (polar_mixed.hip, polar_mixed_tiered.hip): one copy of the
// reference's CMixedKernelListDecoder (out/external/MixedKernelListDecoder.cpp:61-268) over the
// path-index stack of out/external/TVMemoryEngine.cpp:85-142, so both kernels take the same
// decisions with the same tie-breaks and path indices. Also LoadLLRs (chan_llr, every polar
// kernel's) and the wave barrier of every polar kernel. SoftXOR and the mixed kernels' LLR
// routines are in polar_llr_device.h, the tiered kernels' index-table lines in
// polar_tier_device.h. The epilogues stay in the kernels.
//
// One wave per codeword. Lane q < L holds path q's scalars (PathRegs) and slot q of the
// path-index stack in registers; `active` (bit q = path q alive), the stack's top and the
// count k of unfrozen decisions are wave-uniform. What differs per kernel stays there: how a
// phase's LLRs are formed, what a clone copies in LDS, how a decision enters C, the output.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"

namespace bchk {
namespace plist {

// LDS written by some lanes of the wave is read by others after this
__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float rdl_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ uint32_t rdl_u(uint32_t v, int l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint64_t rdl_u64(uint64_t v, int l) {
    return (uint64_t)rdl_u((uint32_t)v, l) | ((uint64_t)rdl_u((uint32_t)(v >> 32), l) << 32);
}

constexpr uint32_t kUninit = 0xFFFFFFFFu;

// The path-index stack of TVMemoryEngine (headers/external/misc.h:212-226) with its lazy
// initialisation: slot i lives in lane i's `slot`, `top` is wave-uniform (pushes and pops are
// v_writelane / v_readlane).
struct PathStack {
    uint32_t slot;
    int top;
    __device__ __forceinline__ void reset(int L, int lane) {
        top = L;
        if (lane == L) slot = kUninit;
    }
    __device__ __forceinline__ uint32_t pop(int lane) {
        const uint32_t v = rdl_u(slot, top);
        if (v == kUninit) {  // never pushed: hand out top - 1
            const int r = top - 1;
            top = r;
            if (r > 0 && lane == r) slot = kUninit;
            return (uint32_t)r;
        }
        --top;
        return v;
    }
    __device__ __forceinline__ void push(uint32_t x, int lane) {
        ++top;
        if (lane == top) slot = x;
    }
};

// path `lane`'s scalars: metric, leaf LLR of the current phase, dynamic-freezing mask and the
// record word (the last k & 31 information bits, flushed to rec every 32 decisions)
struct PathRegs {
    float R, lv;
    uint64_t dm;
    uint32_t rw;
};

// act[k] = index of the k-th active path; returns their number
__device__ __forceinline__ int list_active(uint32_t active, uint32_t *act, int lane, int L) {
    if (lane < L && ((active >> lane) & 1u)) act[__builtin_popcount(active & ((1u << lane) - 1u))] = (uint32_t)lane;
    wsync();
    return __builtin_popcount(active);
}

// the number of valid lanes that come before this one under std::greater<pair<float,
// unsigned>> on (v, lane): larger value first, then the larger index. Ranks the candidates of
// an unfrozen phase (:125) and, with v = R, the final list (:249-267).
__device__ __forceinline__ int rank_greater(float v, bool valid, int lane) {
    int rank = 0;
    for (uint64_t mm = __ballot(valid); mm; mm &= mm - 1) {
        const int o = (int)__builtin_ctzll(mm);
        const float vo = rdl_f(v, o);
        rank += (v < vo || (!(vo < v) && lane < o)) ? 1 : 0;
    }
    return rank;
}

// ---- ContinuePathsFrozen (MixedKernelListDecoder.cpp:61-98): the frozen value from the
// dynamic-freezing mask (phase word e); a path whose LLR says otherwise pays |llr|
__device__ __forceinline__ uint32_t frozen_step(uint32_t e, bool on, PathRegs &r) {
    const int db = (int)((e >> 1) & 127u) - 1;
    uint32_t dec = 0;
    if (on) {
        dec = db >= 0 ? (uint32_t)((r.dm >> db) & 1ull) : 0u;
        if ((dec != 0) ^ (r.lv < 0.0f)) r.R -= fabsf(r.lv);
    }
    return dec;
}

// What becomes of lane's path at an unfrozen phase: cont 1 -> it goes on with bit 0, 2 -> with
// bit 1, 3 -> with the hard decision here and its complement in a clone (`clones`: those
// paths), 0 -> killed (`cont_any`: the paths that go on).
struct Continuations {
    uint32_t cont, cont_any, clones;
};
// ---- ContinuePathsUnfrozen (:100-136). Candidate 2q + b (bit b of path q) sits in lane
// 2q + b; its score is R (b = hard decision) or R - |llr|. The best min(2 nact, L) under the
// reference's std::greater<pair> order (:125) go on; the others' paths are killed, in path
// order (:129-136), their indices pushed.
__device__ __forceinline__ Continuations unfrozen_select(const PathRegs &r, uint32_t &active, int nact,
                                                         PathStack &st, int lane, int L) {
    const int q = lane >> 1, b = lane & 1;
    const float vq = __shfl(r.lv, q & 31), Rq = __shfl(r.R, q & 31);
    const bool valid = q < L && ((active >> q) & 1u);
    float sc = 0.0f;
    if (valid) sc = (b == (vq < 0.0f ? 1 : 0)) ? Rq : Rq - fabsf(vq);
    const int rank = rank_greater(sc, valid, lane);
    const int J = 2 * nact, keep = J < L ? J : L;
    const uint64_t sel = __ballot(valid && rank < keep);
    Continuations c;
    c.cont = lane < L ? (uint32_t)((sel >> (2 * lane)) & 3ull) : 0u;
    c.cont_any = (uint32_t)__ballot(c.cont != 0);
    c.clones = (uint32_t)__ballot(c.cont == 3u);
    for (uint32_t kill = active & ~c.cont_any; kill; kill &= kill - 1) st.push((uint32_t)__builtin_ctz(kill), lane);
    active &= c.cont_any;
    return c;
}
// the bit a continuing path takes itself (:138-178); its score does not change
__device__ __forceinline__ uint32_t own_decision(uint32_t cont, float lv) {
    return cont == 2u ? 1u : (cont == 3u ? (lv < 0.0f ? 1u : 0u) : 0u);
}

// the register half of ClonePath: lane l1 takes path l's scalars and the complement of its
// decision, which costs |llr| (the kernel copies the path's LDS state)
__device__ __forceinline__ void clone_regs(PathRegs &r, uint32_t &dec, int l, int l1, int lane) {
    const float Rl = rdl_f(r.R, l), vl = rdl_f(r.lv, l);
    const uint64_t dml = rdl_u64(r.dm, l);
    const uint32_t rwl = rdl_u(r.rw, l), decl = rdl_u(dec, l);
    if (lane == l1) {
        r.R = Rl - fabsf(vl);
        r.dm = dml;
        r.rw = rwl;
        dec = decl ^ 1u;
        r.lv = vl;
    }
}

// A decision enters a live path's (`now`) scalars, beside the kernel's write into C: the
// dynamic-freezing mask takes the phase's correction (every phase), ...
__device__ __forceinline__ void apply_correction(bool now, uint32_t dec, uint64_t corr, PathRegs &r) {
    if (now && dec) r.dm ^= corr;
}
// ... and an unfrozen phase's bit goes to the record word, flushed to rec[lane * RW + ...] when
// full. (Two calls, placed where the kernels had the statements: one call that tests the phase
// word again cost both kernels about 1 % of their throughput.)
__device__ __forceinline__ void record_decision(bool now, uint32_t dec, PathRegs &r, int &k, uint32_t *rec, int RW,
                                                int lane) {
    if (now) r.rw |= dec << (k & 31);
    ++k;
    if ((k & 31) == 0) {
        if (now) rec[lane * RW + (k >> 5) - 1] = r.rw;
        r.rw = 0;
    }
}
// after the last phase: the partly filled record word
__device__ __forceinline__ void flush_record(const PathRegs &r, int k, bool now, uint32_t *rec, int RW, int lane) {
    if ((k & 31) && now) rec[lane * RW + (k >> 5)] = r.rw;
    wsync();
}

// ---- LoadLLRs (MixedKernelEncoder.cpp:181-207): symbol i of the unshortened code from the
// caller's row y; a shortened symbol is a certain 0, a punctured one an erasure.
__device__ __forceinline__ float chan_llr(const int16_t *symmap, const float *y, int i) {
    const int m = symmap[i];
    return m >= 0 ? y[m] : (m == -1 ? 100000.0f : 0.0f);
}

}  // namespace plist
}  // namespace bchk
