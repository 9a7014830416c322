// polar_mixed.hip -- batched SC-list decoding of polar codes over MIXED binary kernels (Arikan
// layers and matrix kernels, e.g. BCH-derived ones) on gfx950.
//
// Reference: CMixedKernelListDecoder (out/external/MixedKernelListDecoder.cpp:61-268) over
// CListKernelEngine (out/external/KernelListEngine.cpp:266-447); Arikan layers by the f/g of
// SoftProcessing.cpp:39-80; matrix layers by CTrellisKernelProcessor::GetLLRs
// (out/external/TrellisKernelProcessor.cpp:234-294): the offset state accumulates the known
// kernel inputs times their rows, and the LLR of input `phase` is the min-sum difference
// best[1] - best[0] over the coset of the remaining rows (each word's metric a left-to-right
// float sum of |y| over its disagreeing positions -- the trellis's value bit for bit, see
// oracle/polar_oracle.c). Same decisions, arithmetic and path indices as the CPU restatement.
// Layers named G / A5 take their LLRs from the recursive f/g processors of
// TruncatedArikanKernel.cpp:152-184, :341-397 (pllr::named_llrs); their state is part of the
// path (in its S and offset-state strides), so clones and save slots carry it.
//
// Execution model: one wave per codeword (persistent). Every path's S (per layer, outer[λ]
// floats), C (kernel inputs per layer) and matrix offset states live in LDS; lane q < L holds
// path q's scalars (metric, leaf LLR, dynamic-freezing mask, record word, stack slot). A
// matrix LLR's coset is split over lanes when there are fewer (path, element) items than lanes
// (float min is exact, so any split gives the same value). The all-Arikan kernel
// (polar_sclist.hip) stays the fast path for codes without matrix layers.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_list_device.h"
#include "polar_llr_device.h"

namespace bchk {

namespace {

using namespace plist;

// ---- exact kernel LLRs by an ordered-statistics search (matrix kernels beyond the trellis
// limit, e.g. the 64 x 64 extended-BCH kernel of root bchCoder.cpp:356-389 makeMatrix).
// The value is CTrellisKernelProcessor's (:234-294): best[1] - best[0], best[b] the least
// left-to-right float sum of |y| over the disagreeing positions of a word of rows phase+1..l-1
// (b = 0) or of those words plus row `phase` (b = 1). Gauss-Jordan over the positions in
// decreasing |y| gives the most reliable basis of rows phase+1..l-1 (the pivots); a word of
// half b is fixed by its pivot values, and the one matching the hard decision there is the
// root. Flipping a set E of pivots costs at least the sum of their |y| (those positions then
// disagree), so a search over E, cheapest pivot first, that drops every subtree whose flip cost
// exceeds the best metric found (less a float-rounding margin) still visits every word that
// can be a minimum: the result is the coset enumeration's, bit for bit. The wave works on one
// item: 64 lanes sort the positions and eliminate (a lane per row), then evaluate 64 search
// nodes per round (a node per lane) from a LIFO in LDS.
struct MlNode {  // the words c ^ G[i] (and below them): flip cost so far lb, half b
    uint32_t clo, chi;
    uint32_t lbib;  // lb's float bits with the low 7 mantissa bits replaced by i << 1 | b
};                  // (truncating a non-negative float lowers it: still a lower bound)
static_assert(sizeof(MlNode) == kMlNodeBytes, "the stack's stride in LDS and in a save slot");
__device__ __forceinline__ MlNode ml_node(uint64_t c, float lb, int i, int b) {
    return MlNode{(uint32_t)c, (uint32_t)(c >> 32), (__float_as_uint(lb) & ~0x7Fu) | ((uint32_t)i << 1) | (uint32_t)b};
}
struct MlScratch {
    uint64_t *G;   // [64] reduced basis, by increasing flip cost
    uint64_t *U;   // [65] U[i]: non-pivot positions rows i.. can change (suffix unions)
    float *cost;   // [64] flip cost of each basis row (|y| at its pivot)
    float *ay;     // [64] |y| by position
    MlNode *stk;   // [kMlStack]
    // carved out of kMlScratchBytes of LDS at mls (polar_device.h)
    __device__ explicit MlScratch(uint8_t *mls)
        : G(reinterpret_cast<uint64_t *>(mls)), U(reinterpret_cast<uint64_t *>(mls + kMlOffU)),
          cost(reinterpret_cast<float *>(mls + kMlOffCost)), ay(reinterpret_cast<float *>(mls + kMlOffAy)),
          stk(reinterpret_cast<MlNode *>(mls + kMlHeadBytes)) {}
};
// a subtree is dropped when lb * kMlShrink > best: a float sum of at most 64 non-negative terms
// is within 64 u (u = 2^-24) of the exact sum, for lb and for every metric, so the margin
// 2^-15 > 2 * 64 u keeps every word whose float metric could be <= best
constexpr float kMlShrink = 1.0f - 1.0f / 32768.0f;

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
// v from lane ^ J without the LDS crossbar: DPP quad permutes (J = 1, 2), row rotates (J = 4,
// 8) and the gfx950 row / half swaps (J = 16, 32)
template <int J>
__device__ __forceinline__ uint32_t xlane(uint32_t v, int lane) {
    if constexpr (J == 1) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
    } else if constexpr (J == 2) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
    } else if constexpr (J == 4) {
        const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);
        const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x12C, 0xF, 0xF, false);
        return (lane & 4) ? dn : up;
    } else if constexpr (J == 8) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);
    } else if constexpr (J == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (lane & 16) ? r[0] : r[1];
    } else {
        static_assert(J == 32, "lane distance");
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (lane & 32) ? r[0] : r[1];
    }
}
// minimum over the wave of non-negative floats or +inf (their bit patterns order as the
// values do), by DPP / permlane steps
__device__ __forceinline__ float wave_minf(float v) {
    const int lane = (int)__lane_id();
    uint32_t b = __float_as_uint(v), o;
    o = xlane<1>(b, lane);  b = o < b ? o : b;
    o = xlane<2>(b, lane);  b = o < b ? o : b;
    o = xlane<4>(b, lane);  b = o < b ? o : b;
    o = xlane<8>(b, lane);  b = o < b ? o : b;
    o = xlane<16>(b, lane); b = o < b ? o : b;
    o = xlane<32>(b, lane); b = o < b ? o : b;
    return __uint_as_float(b);
}
__device__ __forceinline__ uint64_t wave_xor64(uint64_t v) {
    for (int m = 1; m < 64; m <<= 1) v ^= shfl_xor64(v, m);
    return v;
}
// the metric of the word whose disagreement mask is dis: |y| summed in index order (adding
// +0 where a position agrees leaves the sum unchanged, so this is the trellis's path sum)
// Only the set positions are visited, in ascending order: the +0 terms of the index-order
// sum leave a float sum of non-negative terms unchanged, so the bits are the same, and a lane
// runs popc(dis) steps instead of l.
__device__ __forceinline__ uint64_t ml_below(int l) { return l >= 64 ? ~0ull : ((1ull << l) - 1ull); }
__device__ __forceinline__ float ml_metric(uint64_t dis, const float *ay, int l) {
    float m = 0.0f;
    for (uint64_t v = dis & ml_below(l); v; v &= v - 1) m += ay[__builtin_ctzll(v)];
    return m;
}
// the same, and (fx) the sum over the subset fix of dis
__device__ __forceinline__ void ml_metric2(uint64_t dis, uint64_t fix, const float *ay, int l, float &m, float &fx) {
    m = ml_metric(dis, ay, l);
    fx = ml_metric(fix, ay, l);
}

// A search suspended between two rounds (time-budgeted launches): the wave-uniform state
// beside the scratch (G, U, cost, ay, the stack's first sp nodes), which the caller saves
// and restores with it.
struct MlResume {
    int sp;
    float best0, best1;
    uint64_t hd, lrb;
    uint32_t rounds;  // rounds done so far (the guard below counts the whole search)
};

// rs == null: the whole search in this call. Otherwise *resume says whether the scratch and
// *rs hold a suspended search to continue, and past the deadline (t_launch + budget on the
// 100 MHz clock), after at least one round of this call, the search stops between two rounds:
// *rs filled, *suspended set, the return value meaningless. max_rounds: the guard on the
// search's rounds in all, over every launch it took.
__device__ float ml_llr(const uint64_t *kr, int l, int loc, const float *src, const uint8_t *off, int d, int s,
                        int lane, const MlScratch &ms, uint32_t max_rounds, MlResume *rs = nullptr,
                        bool resume = false, uint64_t t_launch = 0, uint64_t budget = 0,
                        bool *suspended = nullptr) {
    const float kInf = __int_as_float(0x7F800000);
    const uint64_t lt = (1ull << lane) - 1ull;
    const int nf = l - loc - 1;
    uint64_t hd, lrb;
    float best0, best1;
    int sp;
    uint32_t rounds = 0;
    if (rs && resume) {
        hd = rs->hd;
        lrb = rs->lrb;
        best0 = rs->best0;
        best1 = rs->best1;
        sp = rs->sp;
        rounds = rs->rounds;
    } else {
        // the layer's LLRs with the known inputs' sign flips (:240-262), HD = Y < 0 (:270-276)
        float a = 0.0f;
        bool neg = false;
        if (lane < l) {
            const float v = src[lane * d + s];
            const float yv = off[lane * d + s] ? -v : v;
            neg = yv < 0.0f;
            a = fabsf(yv);
            ms.ay[lane] = a;
        }
        hd = __ballot(neg);
        wsync();
        if (nf <= kMlEnumBits) {  // small coset: enumerated, words spread over the lanes
            float b0 = kInf, b1 = kInf;
            for (uint32_t v = (uint32_t)lane; v < (1u << nf); v += 64) {
                uint64_t c = 0;
                for (int r = 0; r < nf; ++r)
                    if ((v >> r) & 1u) c ^= kr[loc + 1 + r];
                const float m0 = ml_metric(c ^ hd, ms.ay, l), m1 = ml_metric(c ^ hd ^ kr[loc], ms.ay, l);
                b0 = m0 < b0 ? m0 : b0;
                b1 = m1 < b1 ? m1 : b1;
            }
            return wave_minf(b1) - wave_minf(b0);
        }
        // positions by decreasing |y| (bitonic across the lanes; key: |y| bits, valid, position)
        uint64_t key = lane < l ? (((uint64_t)__float_as_uint(a) << 8) | 0x80ull | (uint64_t)(63 - lane)) : 0ull;
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint64_t o = shfl_xor64(key, j);
                const bool desc = (lane & k) == 0, lower = (lane & j) == 0;
                key = (lower == desc) ? (o > key ? o : key) : (o < key ? o : key);
            }
        const int pos = 63 - (int)(key & 63ull);
        // Gauss-Jordan: lane i < nf holds row loc + 1 + i; pivots in decreasing |y|
        uint64_t g = lane < nf ? kr[loc + 1 + lane] : 0ull;
        bool used = false;
        int t = 0, piv = 0;
        for (int si = 0, np = 0; si < l && np < nf; ++si) {
            const int p = __builtin_amdgcn_readlane(pos, si);
            const uint64_t cand = __ballot(lane < nf && !used && ((g >> p) & 1ull));
            if (!cand) continue;
            const int r = (int)__builtin_ctzll(cand);
            const uint64_t gr = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)g, r) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(g >> 32), r) << 32);
            if (lane == r) {
                used = true;
                t = np;
                piv = p;
            } else if (lane < nf && ((g >> p) & 1ull)) {
                g ^= gr;
            }
            ++np;
        }
        if (lane < nf) {  // found in decreasing |y|: index nf - 1 - t runs by increasing cost
            ms.G[nf - 1 - t] = g;
            ms.cost[nf - 1 - t] = ms.ay[piv];
        }
        // non-pivot positions; below a word that has taken rows up to i - 1, every non-pivot
        // disagreement outside U[i] is fixed, so its |y| bounds the subtree from below too
        uint64_t pm = lane < nf ? (1ull << piv) : 0ull;
        for (int o = 1; o < 64; o <<= 1) pm |= shfl_xor64(pm, o);
        lrb = ~pm & (l >= 64 ? ~0ull : ((1ull << l) - 1ull));
        wsync();
        if (lane <= nf) {
            uint64_t u = 0ull;
            for (int q = lane; q < nf; ++q) u |= ms.G[q] & lrb;
            ms.U[lane] = u;
        }
        // the roots: the word of each half that matches the hard decision on the pivots
        const uint64_t root0 = wave_xor64(lane < nf && ((hd >> piv) & 1ull) ? g : 0ull);
        const uint64_t t1 = hd ^ kr[loc];
        const uint64_t root1 = kr[loc] ^ wave_xor64(lane < nf && ((t1 >> piv) & 1ull) ? g : 0ull);
        best0 = ml_metric(root0 ^ hd, ms.ay, l);
        best1 = ml_metric(root1 ^ hd, ms.ay, l);
        if (lane == 0) {
            ms.stk[0] = ml_node(root0, 0.0f, 0, 0);
            ms.stk[1] = ml_node(root1, 0.0f, 0, 1);
        }
        sp = 2;
        wsync();
    }
    // a guard only (the search tree is finite): past max_rounds rounds (2^20; counted over
    // every launch the search took) the LLR is NaN, never a hang
    for (const uint32_t first = rounds; sp > 0; ++rounds) {
        if (rounds >= max_rounds) return __int_as_float(0x7FC00000);
        if (rs && rounds > first && __builtin_amdgcn_s_memrealtime() - t_launch > budget) {
            rs->sp = sp;  // past the launch's deadline: stop between two rounds
            rs->best0 = best0;
            rs->best1 = best1;
            rs->hd = hd;
            rs->lrb = lrb;
            rs->rounds = rounds;
            *suspended = true;
            return 0.0f;
        }
        // the top n nodes, one per lane; n shrinks near the stack's end so that the pushes of a
        // round (at most 2 per node) and of one depth-first descent (< 64) always fit
        int n = sp < 64 ? sp : 64;
        const int room = kMlStack - 128 - sp;
        if (room < n) n = room > 1 ? room : 1;
        const bool have = lane < n;
        MlNode e{0u, 0u, 0u};
        if (have) e = ms.stk[sp - n + lane];
        sp -= n;
        wsync();
        const uint64_t ec = (uint64_t)e.clo | ((uint64_t)e.chi << 32);
        const float elb = __uint_as_float(e.lbib & ~0x7Fu);
        const int i = (int)((e.lbib >> 1) & 63u);
        const bool hb = (e.lbib & 1u) != 0;
        const float bound = hb ? best1 : best0;
        const float l2 = have ? elb + ms.cost[i] : kInf;
        const bool live = have && l2 * kMlShrink <= bound;
        uint64_t c2 = 0ull;
        float m = kInf, fx = 0.0f;
        if (live) {
            c2 = ec ^ ms.G[i];
            const uint64_t dis = c2 ^ hd;
            ml_metric2(dis, dis & lrb & ~ms.U[i + 1], ms.ay, l, m, fx);
        }
        const float n0 = wave_minf(live && !hb ? m : kInf), n1 = wave_minf(live && hb ? m : kInf);
        best0 = n0 < best0 ? n0 : best0;
        best1 = n1 < best1 ? n1 : best1;
        const float nb = hb ? best1 : best0;
        const bool more = live && i + 1 < nf;
        const float nc = more ? ms.cost[i + 1] : 0.0f;
        const bool psib = more && (elb + nc) * kMlShrink <= nb;     // the next pivot instead of this one
        const bool pch = more && (l2 + fx + nc) * kMlShrink <= nb;  // this one and a later one
        const uint64_t ms_ = __ballot(psib), mc = __ballot(pch);
        const int nsib = __builtin_popcountll(ms_);
        if (psib) ms.stk[sp + __builtin_popcountll(ms_ & lt)] = ml_node(ec, elb, i + 1, hb ? 1 : 0);
        if (pch) ms.stk[sp + nsib + __builtin_popcountll(mc & lt)] = ml_node(c2, l2, i + 1, hb ? 1 : 0);
        sp += nsib + __builtin_popcountll(mc);
        wsync();
    }
    return best1 - best0;  // (:292)
}

// A wave-uniform value that came through a vector load, into scalar registers.
// (readfirstlane returns int: through uint32_t, or a low word sign-extends)
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float uni(float v) { return __uint_as_float(uni(__float_as_uint(v))); }
__device__ __forceinline__ uint64_t uni(uint64_t v) {
    return (uint64_t)uni((uint32_t)v) | ((uint64_t)uni((uint32_t)(v >> 32)) << 32);
}

// ---- a save slot's LDS regions (polar_device.h PolarSaveHeader), one routine for both
// directions so that suspend and resume cannot drift: kSave copies LDS to the slot, else the
// slot to LDS, as 32-bit words. The caller issues wsync() before other lanes read restored LDS.
template <bool kSave>
__device__ __forceinline__ void slot_copy(uint8_t *slot, uint8_t *lds, int bytes, int lane) {
    for (int i = 4 * lane; i < bytes; i += 256) {
        uint32_t *g = reinterpret_cast<uint32_t *>(slot + i), *l = reinterpret_cast<uint32_t *>(lds + i);
        if (kSave) *g = *l;
        else *l = *g;
    }
}
// the list state: channel / S / C / O, and act / rec
template <bool kSave>
__device__ __forceinline__ void slot_list_state(uint8_t *sv, uint8_t *smem, const PolarMixedLayout &lo, int lane) {
    slot_copy<kSave>(sv + kSaveLdsOff, smem, lo.o_ph, lane);
    slot_copy<kSave>(sv + lo.sv_act, smem + lo.o_act, lo.o_tm - lo.o_act, lane);
}
// a suspended search's scratch at mls: G, U, cost, ay and the stack's first sp nodes
template <bool kSave>
__device__ __forceinline__ void slot_search(uint8_t *sv, uint8_t *mls, const PolarMixedLayout &lo, int sp, int lane) {
    slot_copy<kSave>(sv + lo.sv_ml, mls, (int)kMlHeadBytes + (int)kMlNodeBytes * sp, lane);
}

}  // namespace

__global__ void __launch_bounds__(64) polar_mixed_kernel(PolarMixedParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = (int)threadIdx.x;
    const int U = p.U, nl = p.nl, L = p.L, K = p.K;
    const int RW = polar_rec_words(K);
    // LDS: polar_mixed_layout (polar_device.h)
    const PolarMixedLayout lo = polar_mixed_layout(U, L, K, p.ssize, p.csize, p.osize, nl, p.tstates, p.any_ml != 0);
    float *chan = reinterpret_cast<float *>(smem);
    float *S = reinterpret_cast<float *>(smem + lo.o_S);
    uint8_t *C = smem + lo.o_C;
    uint8_t *O = smem + lo.o_O;
    uint16_t *ph = reinterpret_cast<uint16_t *>(smem + lo.o_ph);
    uint64_t *rows = reinterpret_cast<uint64_t *>(smem + lo.o_rows);  // [layer][row] bitmasks
    uint32_t *act = reinterpret_cast<uint32_t *>(smem + lo.o_act);
    uint32_t *rec = act + L;
    float *tmet = reinterpret_cast<float *>(smem + lo.o_tm);  // trellis state metrics, 2 x tstates
    uint8_t *mls = smem + lo.o_ml;  // ordered-statistics search scratch
    const MlScratch ms(mls);
    const bool mine = lane < L;
    for (int i = lane; i < U; i += 64) ph[i] = p.io.phase[i];
    for (int i = lane; i < kPolarMaxKernel * nl; i += 64) rows[i] = p.krows[i];
    auto Sof = [&](int q, int lam) -> float * { return lam == 0 ? chan : S + (size_t)q * p.ssize + p.soff[lam]; };
    auto Cof = [&](int q, int lam) -> uint8_t * { return C + (size_t)q * p.csize + p.coff[lam]; };
    auto Oof = [&](int q, int j) -> uint8_t * { return O + (size_t)q * p.osize + p.ooff[j]; };
    auto Fof = [&](int q, int j) -> float * { return S + (size_t)q * p.ssize + p.foff[j]; };  // named layers' state
    auto pathof = [&](int k) -> int { return (int)act[k]; };  // the k-th active path
    const pllr::Trellis tr{p.tent, p.tbase, p.tlog, tmet, p.tstates};
    const int lastsz = p.ksize[nl - 1];
    const int lastc = p.coff[nl];
    PathStack st;
    st.slot = 0;
    wsync();
    // time-budgeted launches (PolarMixedParams::budget): this launch's start on the 100 MHz clock
    const bool budgeted = p.budget != 0 && p.rstate != nullptr;
    const uint64_t t_launch = __builtin_amdgcn_s_memrealtime();
    auto expired = [&]() { return budgeted && __builtin_amdgcn_s_memrealtime() - t_launch > p.budget; };
    // Liveness under any budget: the first unfinished codeword a wave meets in a launch is
    // started (or resumed) whatever the clock says, so the clock only stops a wave that has
    // worked in this launch. `stop` is sticky: after a suspension or the first skip the wave
    // starts nothing more, so the codewords of its stride are, in order, finished ones, at most
    // one suspended one, then untouched ones -- which is what lets the save slot be the wave's.
    bool worked = false, stop = false;
    uint32_t prog = 0;  // search rounds (one counted per suspended search), items, codewords done
    uint8_t *const sv = budgeted ? p.rsave + (size_t)blockIdx.x * p.rstride : nullptr;
    for (uint32_t cw = blockIdx.x; cw < p.B; cw += gridDim.x) {
        const uint32_t cst = budgeted ? __builtin_amdgcn_readfirstlane(p.rstate[cw]) : 0u;
        if (cst == 2u) continue;  // finished by an earlier launch
        if (stop || (worked && expired())) {  // past the budget: start (or resume) nothing more
            stop = true;
            if (lane == 0) atomicAdd(p.unfinished, 1u);
            continue;
        }
        worked = true;
        uint32_t active;
        PathRegs pr{0.0f, 0.0f, 0ull, 0u};
        int k = 0, phi0 = 0, rj = -1, rit = 0;  // rj >= 0: resume in layer rj at item rit
        MlResume mr{0, 0.0f, 0.0f, 0ull, 0ull, 0u};
        bool rmid = false;  // resuming inside a search item (its scratch saved too)
        if (cst == 1u) {
            // resume a suspended codeword: header, registers, the list state's LDS
            const PolarSaveHeader h = *reinterpret_cast<const PolarSaveHeader *>(sv);
            phi0 = (int)uni(h.phi);
            rj = (int)uni(h.layer);
            rit = (int)uni(h.item);
            k = (int)uni(h.k);
            active = uni(h.active);
            st.top = (int)uni(h.top);
            const PolarSaveLane g = reinterpret_cast<const PolarSaveLane *>(sv + kSaveHeaderBytes)[lane];
            pr = PathRegs{g.R, g.lv, g.dm, g.rw};
            st.slot = g.slot;
            slot_list_state<false>(sv, smem, lo, lane);
            rmid = uni(h.mid) != 0u;
            if (rmid) {
                mr = MlResume{(int)uni(h.sp), uni(h.best0), uni(h.best1), uni(h.hd), uni(h.lrb), uni(h.rounds)};
                slot_search<false>(sv, mls, lo, mr.sp, lane);
            }
        } else {
            const float *y = p.io.llr + (size_t)cw * p.N;  // LoadLLRs (MixedKernelEncoder.cpp:181-207)
            for (int i = lane; i < U; i += 64) chan[i] = chan_llr(p.io.symmap, y, i);
            st.reset(L, lane);
            const uint32_t pid = st.pop(lane);
            active = 1u << pid;
        }
        wsync();
        int nact = list_active(active, act, lane, L);
        bool progressed = false, yielded = false;
        // suspend between two search items (the list state is complete there: every layer
        // before rj done, layer rj's offset state applied, items before it done), or (mid)
        // inside a search item, whose scratch and MlResume go along
        auto suspend = [&](int phi, int j, int it, bool mid) {
            if (lane == 0)
                *reinterpret_cast<PolarSaveHeader *>(sv) =
                    PolarSaveHeader{(uint32_t)phi, (uint32_t)j, (uint32_t)it, (uint32_t)k, active, (uint32_t)st.top,
                                    mid ? 1u : 0u, (uint32_t)mr.sp, mr.best0, mr.best1, mr.hd, mr.lrb, mr.rounds};
            if (mid) slot_search<true>(sv, mls, lo, mr.sp, lane);
            reinterpret_cast<PolarSaveLane *>(sv + kSaveHeaderBytes)[lane] = PolarSaveLane{pr.R, pr.lv, pr.dm, pr.rw, st.slot};
            slot_list_state<true>(sv, smem, lo, lane);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            if (lane == 0) {
                p.rstate[cw] = 1u;
                atomicAdd(p.unfinished, 1u);
                if (prog) atomicAdd(p.progress, prog);
            }
            prog = 0;
            yielded = true;
            stop = true;
        };
        for (int phi = phi0; phi < U && !yielded; ++phi) {
            const uint32_t e = __builtin_amdgcn_readfirstlane((uint32_t)ph[phi]);
            // ---- IterativelyCalcS (KernelListEngine.cpp:370-447)
            int m = nl - 1;
            uint32_t pq = (uint32_t)phi;
            while (m > 0 && pq % (uint32_t)p.ksize[m] == 0) {
                pq /= (uint32_t)p.ksize[m];
                --m;
            }
            for (int j = m; j < nl; ++j) {
                if (rj >= 0 && j < rj) continue;  // done before the suspension
                const bool resume_here = rj == j;
                const int loc = (j == m) ? (int)(pq % (uint32_t)p.ksize[j]) : 0;
                const int d = p.outer[j + 1], l = p.ksize[j];
                const int tot = nact * d;
                if (p.arikan[j]) {
                    pllr::arikan_llrs(j, loc, d, tot, lane, pathof, Sof, Cof);
                    wsync();
                    continue;
                }
                if (p.named[j]) {  // G / A5: the f/g processor over the path's carried state
                    pllr::named_llrs(p.named[j], j, loc, d, tot, lane, pathof, Sof, Cof, Fof, Oof);
                    wsync();
                    continue;
                }
                // matrix layer: offset state (:240-262), then the min-sum LLR per element
                const uint64_t *kr = rows + kPolarMaxKernel * j;
                if (!resume_here) pllr::matrix_offsets(kr, j, l, loc, d, tot, lane, pathof, Cof, Oof);  // (applied before a suspension)
                wsync();
                if (p.ml[j]) {
                    // exact ordered-statistics search (kernels larger than the trellis limit):
                    // one item at a time, the whole wave on it
                    for (int it = resume_here ? rit : 0; it < tot; ++it) {
                        if (progressed && expired()) {  // past the launch's budget: suspend here
                            suspend(phi, j, it, false);
                            break;
                        }
                        const int q = (int)act[it / d], s = it % d;
                        const bool mid = resume_here && it == rit && rmid;  // continue a suspended search
                        bool susp = false;
                        const float v = ml_llr(kr, l, loc, Sof(q, j), Oof(q, j), d, s, lane, ms, p.ml_rounds,
                                               budgeted && !p.no_mid ? &mr : nullptr, mid, t_launch, p.budget,
                                               &susp);
                        ++prog;      // the item, or (suspended) the one round or more it ran
                        if (susp) {  // the search itself ran past the budget: suspended inside it
                            suspend(phi, j, it, true);
                            break;
                        }
                        if (lane == 0) Sof(q, j + 1)[s] = v;
                        wsync();
                        progressed = true;
                    }
                    rj = -1;
                    if (yielded) break;
                    continue;
                }
                if (p.trellis[j]) {
                    pllr::trellis_llrs(tr, j, l, loc, d, tot, lane, pathof, Sof, Oof);
                    continue;
                }
                pllr::enum_llrs(kr, j, l, loc, d, tot, lane, pathof, Sof, Oof);
                wsync();
            }
            if (yielded) break;
            const bool on = mine && ((active >> lane) & 1u);
            if (on) pr.lv = Sof(lane, nl)[0];
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
                    const int l1 = (int)st.pop(lane);  // ClonePath: the whole path state
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
            if (now) {
                C[(size_t)lane * p.csize + lastc + (phi % lastsz)] = (uint8_t)dec;
                apply_correction(now, dec, corr, pr);
            }
            if (!(e & kPhaseFrozen)) {
                record_decision(now, dec, pr, k, rec, RW, lane);
                nact = list_active(active, act, lane, L);
            } else {
                wsync();
            }
            // ---- IterativelyUpdateC (KernelListEngine.cpp:266-315): finished blocks are
            // multiplied by their kernel into the parent layer's inputs
            pllr::update_c(rows, p.ksize, nl, phi, nact, lane, pathof, Cof);
        }
        if (yielded) {  // suspended: outputs when it finishes in a later launch
            wsync();
            continue;
        }
        const bool me = mine && ((active >> lane) & 1u);
        flush_record(pr, k, me, rec, RW, lane);
        // ---- final order (:249-267): active paths by (R, index), descending
        const int rk = rank_greater(pr.R, me, lane);
        for (int r = 0; r < nact; ++r) {
            const int q = (int)__builtin_ctzll(__ballot(me && rk == r));
            const uint8_t *cq = C + (size_t)q * p.csize;  // C_0: the unshortened codeword
            const uint32_t *rq = rec + q * RW;
            const size_t row = (size_t)cw * L + r;
            for (int kk = lane; kk < K; kk += 64) p.io.info[row * K + kk] = (uint8_t)((rq[kk >> 5] >> (kk & 31)) & 1u);
            if (p.io.cw)
                for (int i = lane; i < p.N; i += 64) p.io.cw[row * p.N + i] = cq[p.io.cwpos[i]];
            if (lane == 0) p.io.metric[row] = rdl_f(pr.R, q);
        }
        if (lane == 0) p.io.count[cw] = nact;
        if (budgeted && lane == 0) {
            p.rstate[cw] = 2u;
            atomicAdd(p.progress, prog + 1u);
        }
        prog = 0;
        wsync();
    }
}

hipError_t launch_polar_mixed(const PolarMixedParams &p, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(polar_mixed_kernel, dim3(grid), dim3(64), lds, s, p);
    return hipGetLastError();
}

const void *polar_mixed_kernel_ptr() { return reinterpret_cast<const void *>(&polar_mixed_kernel); }

}  // namespace bchk
