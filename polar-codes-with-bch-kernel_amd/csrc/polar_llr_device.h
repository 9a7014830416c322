// polar_llr_device.h -- the per-layer LLR and partial-sum routines of SC decoding over mixed
// kernels, shared by the SC-list kernels (polar_mixed.hip, polar_mixed_tiered.hip) and the genie-aided single-path
// kernel (polar_genie.hip): one copy of the arithmetic, so both give the same bits.
//
// Arikan layers: the f/g of SoftProcessing.cpp:39-80. Matrix layers:
// CTrellisKernelProcessor::GetLLRs (out/external/TrellisKernelProcessor.cpp:234-294): the
// offset state accumulates the known kernel inputs times their rows, and the LLR of input
// `phase` is the min-sum difference best[1] - best[0] over the coset of the remaining rows,
// by coset enumeration or by the pull-form Viterbi over the trellis. Named layers (G, A5):
// the recursive f/g processors of TruncatedArikanKernel.cpp with their per-path state. Partial
// sums: IterativelyUpdateC (KernelListEngine.cpp:266-315). soft_xor is the only SoftXOR of the
// polar kernels: the all-Arikan kernels (polar_sclist.hip, polar_sclist_tiered.hip) call it too.
//
// The routines run on one wave. Work items are (path, element) pairs, it = k * d + s with k
// an index into the caller's active paths: pathof(k) is the path, Sof(q, λ) its LLRs of layer
// λ, Cof(q, λ) its kernel inputs of layer λ, Oof(q, j) its offset state of matrix layer j.
// A caller with one path passes pathof = 0. Unless stated, the caller issues wsync() before
// other lanes read what a routine wrote.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_list_device.h"

namespace bchk {
namespace pllr {

using plist::wsync;

// min over the words of one half of the coset (CTrellisKernelProcessor::GetLLRs, :272-292):
// words c = XOR of rows phase+1 .. l-1 selected by v, v = first, first + step, ...; metric of
// c (b = 0) and c ^ row[phase] (b = 1) against the hard decision (l <= 32)
__device__ __forceinline__ void coset_min(const uint64_t *rows, int l, int phase, const float *ay, uint64_t hd,
                                          uint32_t first, uint32_t step, float &b0, float &b1) {
    const int nfree = l - phase - 1;
    const uint32_t nw = 1u << nfree;
    for (uint32_t v = first; v < nw; v += step) {
        uint64_t c = 0;
        for (int r = 0; r < nfree; ++r)
            if ((v >> r) & 1u) c ^= rows[phase + 1 + r];
        const uint64_t d0 = c ^ hd, d1 = d0 ^ rows[phase];
        float m0 = 0.0f, m1 = 0.0f;  // left to right (:279-282)
        for (int j = 0; j < l; ++j) {
            if ((d0 >> j) & 1ull) m0 += ay[j];
            if ((d1 >> j) & 1ull) m1 += ay[j];
        }
        b0 = m0 < b0 ? m0 : b0;
        b1 = m1 < b1 ? m1 : b1;
    }
}

// SoftXOR and SoftCombine of one element (SoftProcessing.cpp:54-80, :39-50): the one spelling of
// both in the polar kernels. SoftXOR: sign(a) sign(b) min(|a|, |b|)
__device__ __forceinline__ float soft_xor(float a, float b) {
    const float fa = fabsf(a), fb = fabsf(b), mn = fa < fb ? fa : fb;
    return __uint_as_float(__float_as_uint(mn) | ((__float_as_uint(a) ^ __float_as_uint(b)) & 0x80000000u));
}
__device__ __forceinline__ float soft_combine(float a, float b, uint32_t c) { return c ? b - a : b + a; }

// Arikan layer j at local phase loc: S_{j+1} from S_j (d = outer[j + 1] elements per path)
template <class PathOf, class SOf, class COf>
__device__ __forceinline__ void arikan_llrs(int j, int loc, int d, int tot, int lane, PathOf pathof, SOf Sof,
                                            COf Cof) {
    for (int it = lane; it < tot; it += 64) {
        const int q = pathof(it / d), s = it % d;
        const float *src = Sof(q, j);
        float *dst = Sof(q, j + 1);
        const float a = src[s], b = src[d + s];
        dst[s] = loc ? soft_combine(a, b, Cof(q, j + 1)[s]) : soft_xor(a, b);
    }
}

// Named layer j (kind kNamedG / kNamedA5, polar_device.h) at local phase loc:
// CGKernelProcessor::GetLLRs and CA5KernelProcessor::GetLLRs (out/external/
// TruncatedArikanKernel.cpp:152-184, :341-397), operation for operation. y_i = Sof(q, j)[i d + s]
// are the layer's LLRs, u_i = Cof(q, j + 1)[i d + s] its known inputs; the state of element s
// (Fof(q, j): floats, stride d per variable; Oof(q, j): A5's bit) is the path's own, written by
// the lane that reads it at a later phase, so it travels with every clone of the path.
template <class PathOf, class SOf, class COf, class FOf, class OOf>
__device__ __forceinline__ void named_llrs(int kind, int j, int loc, int d, int tot, int lane, PathOf pathof, SOf Sof,
                                           COf Cof, FOf Fof, OOf Oof) {
    for (int it = lane; it < tot; it += 64) {
        const int q = pathof(it / d), s = it % d;
        const float *y = Sof(q, j) + s;
        const uint8_t *u = Cof(q, j + 1) + s;
        float *st = Fof(q, j) + s;
        float r;
        if (kind == kNamedG) {  // state: L1 [+] L2
            if (loc == 0) {     // (:163-169)
                const float l12 = soft_xor(y[d], y[2 * d]);
                st[0] = l12;
                r = soft_xor(y[0], l12);
            } else if (loc == 1) {  // (:170-175)
                r = soft_combine(y[0], st[0], u[0]);
            } else {  // (:176-181)
                r = soft_combine(y[d], y[2 * d], u[d]);
            }
        } else {  // A5; state: L04, L13, L024 and the bit pC
            float *l04 = st, *l13 = st + d, *l024 = st + 2 * d;
            uint8_t *pc = Oof(q, j) + s;
            if (loc == 0) {  // (:357-364)
                const float a = soft_xor(y[0], y[4 * d]);
                const float b = soft_xor(a, y[2 * d]);
                const float c = soft_xor(y[d], y[3 * d]);
                *l04 = a;
                *l024 = b;
                *l13 = c;
                r = soft_xor(b, c);
            } else if (loc == 1) {  // (:365-369)
                r = soft_combine(*l024, *l13, u[0]);
            } else if (loc == 2) {  // (:370-377)
                const uint32_t c = (u[0] ^ u[d]) & 1u;
                const float b = soft_combine(*l04, y[2 * d], c);
                const float e = soft_combine(y[d], y[3 * d], u[d]);
                *pc = (uint8_t)c;
                *l024 = b;
                *l13 = e;
                r = soft_xor(b, e);
            } else if (loc == 3) {  // (:378-387)
                const float e = soft_combine(y[2 * d], soft_combine(y[d], y[3 * d], u[d]), u[2 * d]);
                const float a = soft_xor(y[0], e);
                const uint32_t c = (*pc ^ u[2 * d]) & 1u;
                *l13 = e;
                *l04 = a;
                *pc = (uint8_t)c;
                r = soft_combine(a, y[4 * d], c);
            } else {  // (:388-393)
                const uint32_t c = (*pc ^ u[3 * d]) & 1u;
                *pc = (uint8_t)c;
                r = soft_combine(y[0], *l13, c);
            }
        }
        Sof(q, j + 1)[s] = r;
    }
}

// matrix layer j (rows kr, size l) at local phase loc: the offset state (:240-262), cleared at
// phase 0, then XORed with row loc - 1 where the input decided last is 1
template <class PathOf, class COf, class OOf>
__device__ __forceinline__ void matrix_offsets(const uint64_t *kr, int j, int l, int loc, int d, int tot, int lane,
                                               PathOf pathof, COf Cof, OOf Oof) {
    for (int it = lane; it < tot; it += 64) {
        const int q = pathof(it / d), s = it % d;
        uint8_t *off = Oof(q, j);
        if (!loc) {
            for (int i = 0; i < l; ++i) off[i * d + s] = 0;
        } else {
            const uint8_t kn = Cof(q, j + 1)[(loc - 1) * d + s];
            if (kn)
                for (int i = 0; i < l; ++i)
                    if ((kr[loc - 1] >> i) & 1ull) off[i * d + s] ^= 1u;
        }
    }
}

// the trellis tables of a context (polar_device.h) and the wave's two metric buffers
struct Trellis {
    const uint32_t *tent, *tbase;
    const uint8_t *tlog;
    float *tmet;  // LDS, 2 x tstates floats
    int tstates;
};

// matrix layer j's LLRs through its trellis: CTrellisKernelProcessor::GetLLRs (:260-292) as a
// pull-form Viterbi: a state of depth dd + 1 takes the smaller of its (at most two)
// predecessors' metrics, each plus |Y| when its edge label differs from the hard decision (min
// commutes with the monotone float add, so the values are the reference's). G lanes per item
// (G = states of the phase's widest depth, at most 64). Synchronises itself.
template <class PathOf, class SOf, class OOf>
__device__ __forceinline__ void trellis_llrs(const Trellis &tr, int j, int l, int loc, int d, int tot, int lane,
                                             PathOf pathof, SOf Sof, OOf Oof) {
    const int tp = j * kPolarMaxKernel + loc;
    const uint8_t *lgp = tr.tlog + (size_t)tp * (kPolarMaxKernel + 1);
    const uint32_t *ent0 = tr.tent + tr.tbase[tp];
    int ab = 0;
    for (int dd = 1; dd <= l; ++dd) ab = lgp[dd] > ab ? lgp[dd] : ab;
    const int stride = 1 << ab, G = stride < 64 ? stride : 64, ipr = 64 / G;
    const int slot = lane / G, sub = lane % G;
    for (int base = 0; base < tot; base += ipr) {
        const int it = base + slot;
        const bool have = slot < ipr && it < tot;
        int q = 0, s = 0;
        if (have) {
            q = pathof(it / d);
            s = it % d;
        }
        const float *src = Sof(q, j);
        const uint8_t *off = Oof(q, j);
        float *m0 = tr.tmet + slot * stride, *m1 = tr.tmet + tr.tstates + slot * stride;
        if (have && sub == 0) m0[0] = 0.0f;
        wsync();
        const uint32_t *e = ent0;
        for (int dd = 0; dd < l; ++dd) {
            const int n1 = 1 << lgp[dd + 1];
            if (have) {
                const float v = src[dd * d + s];
                const float yv = off[dd * d + s] ? -v : v;
                const bool hd = yv < 0.0f;  // HD = Y < 0 (:270)
                const float ay = fabsf(yv);
                for (int S1 = sub; S1 < n1; S1 += G) {
                    const uint32_t w = e[S1], a = w & 0xFFFFu, b = w >> 16;
                    float x = m0[a & kTrellisState];
                    if (((a & kTrellisZ) != 0u) != hd) x = x + ay;
                    if (b & kTrellisValid) {
                        float xb = m0[b & kTrellisState];
                        if (((b & kTrellisZ) != 0u) != hd) xb = xb + ay;
                        x = xb < x ? xb : x;
                    }
                    m1[S1] = x;
                }
            }
            wsync();
            float *tt = m0;
            m0 = m1;
            m1 = tt;
            e += n1;
        }
        if (have && sub == 0) Sof(q, j + 1)[s] = m0[1] - m0[0];  // (:292)
        wsync();
    }
}

// matrix layer j's LLRs by coset enumeration (l <= 32); the coset is split over lanes when
// items are fewer than lanes (float min is exact, so any split gives the same value)
template <class PathOf, class SOf, class OOf>
__device__ __forceinline__ void enum_llrs(const uint64_t *kr, int j, int l, int loc, int d, int tot, int lane,
                                          PathOf pathof, SOf Sof, OOf Oof) {
    int lpi = 1;
    const int nfree = l - loc - 1;
    while (lpi * 2 * tot <= 64 && (lpi * 2) <= (1 << (nfree < 6 ? nfree : 6))) lpi *= 2;
    const int span = 64 / lpi * lpi;  // lanes used per round
    for (int base = 0; base < tot * lpi; base += span) {
        const int g = base + lane;
        const bool have = lane < span && g < tot * lpi;
        const int it = g / lpi, sub = g % lpi;
        float b0 = __int_as_float(0x7F800000), b1 = __int_as_float(0x7F800000);
        int q = 0, s = 0;
        if (have) {
            q = pathof(it / d);
            s = it % d;
            const float *src = Sof(q, j);
            const uint8_t *off = Oof(q, j);
            float ay[kPolarMaxTrellisKernel];  // enumerated layers: l <= 32
            uint64_t hd = 0;
            for (int jj = 0; jj < l; ++jj) {
                const float v = src[jj * d + s];
                const float yv = off[jj * d + s] ? -v : v;
                if (yv < 0.0f) hd |= 1ull << jj;  // HD = Y < 0 (:276)
                ay[jj] = fabsf(yv);
            }
            coset_min(kr, l, loc, ay, hd, (uint32_t)sub, (uint32_t)lpi, b0, b1);
        }
        for (int o = 1; o < lpi; o <<= 1) {  // min over the item's lanes (exact)
            const float x0 = __shfl_xor(b0, o, 64), x1 = __shfl_xor(b1, o, 64);
            b0 = x0 < b0 ? x0 : b0;
            b1 = x1 < b1 ? x1 : b1;
        }
        if (have && sub == 0) Sof(q, j + 1)[s] = b1 - b0;  // (:292)
    }
}

// IterativelyUpdateC (KernelListEngine.cpp:266-315) after input phi of the last layer is
// set in every active path: finished blocks are multiplied by their kernel into the parent
// layer's inputs. rows: [layer][kPolarMaxKernel] bitmasks. Synchronises after each layer.
template <class PathOf, class COf>
__device__ __forceinline__ void update_c(const uint64_t *rows, const int32_t *ksize, int nl, int phi, int nact,
                                         int lane, PathOf pathof, COf Cof) {
    int lam = nl, stride = 1;
    uint32_t ph2 = (uint32_t)phi;
    while (lam > 0 && (ph2 + 1) % (uint32_t)ksize[lam - 1] == 0) {
        const int l = ksize[lam - 1];
        const uint32_t psi = ph2 / (uint32_t)l;
        const int next = stride * l;
        const int phi0 = lam > 1 ? (int)(psi % (uint32_t)ksize[lam - 2]) * next : 0;
        const uint64_t *kr = rows + kPolarMaxKernel * (lam - 1);
        const int tot = nact * stride;
        for (int it = lane; it < tot; it += 64) {
            const int q = pathof(it / stride), s = it % stride;
            const uint8_t *x = Cof(q, lam);
            uint8_t *yo = Cof(q, lam - 1) + phi0;
            // (y_i) = (x_j) K: y_i = XOR over rows j with K[j][i] (LinAlg.cpp:685-709)
            uint64_t yv = 0;
            for (int jj = 0; jj < l; ++jj)
                if (x[jj * stride + s] & 1u) yv ^= kr[jj];
            for (int i = 0; i < l; ++i) yo[i * stride + s] = (uint8_t)((yv >> i) & 1ull);
        }
        wsync();
        stride = next;
        ph2 = psi;
        --lam;
    }
}

// One layer of update_c's loop, its arithmetic restated, for a caller whose C_λ and C_{λ-1} lie
// in different memories (polar_mixed_tiered.hip; update_c itself stays as it is, so the kernels
// that call it compile as before): the finished block of C_λ (Xof(q): l inputs of `stride`
// elements each; kr the kernel's rows) times the kernel, into Yof(q) = C_{λ-1} from byte phi0 on.
// No synchronisation.
template <class PathOf, class XOf, class YOf>
__device__ __forceinline__ void update_c_layer(const uint64_t *kr, int l, int stride, int phi0, int nact, int lane,
                                               PathOf pathof, XOf Xof, YOf Yof) {
    const int tot = nact * stride;
    for (int it = lane; it < tot; it += 64) {
        const int q = pathof(it / stride), s = it % stride;
        const uint8_t *x = Xof(q);
        uint8_t *yo = Yof(q) + phi0;
        // (y_i) = (x_j) K: y_i = XOR over rows j with K[j][i] (LinAlg.cpp:685-709)
        uint64_t yv = 0;
        for (int jj = 0; jj < l; ++jj)
            if (x[jj * stride + s] & 1u) yv ^= kr[jj];
        for (int i = 0; i < l; ++i) yo[i * stride + s] = (uint8_t)((yv >> i) & 1ull);
    }
}

}  // namespace pllr
}  // namespace bchk
