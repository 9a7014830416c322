// kernel_bec.hip -- BEC polarisation behaviour of a polar kernel on the GPU, behind the
// bchk_kernel_bec_* C ABI (include/bchk.h): which input phases an erasure pattern leaves
// undecodable, counted by erasure weight. This is the producer of the per-kernel table the
// reference only consumes (CBECCapacityEvaluator, out/external/CapacityEvaluator.cpp:100-140;
// the "3" section of a kernel file, Kernel.cpp:113-134).
//
// Conventions are the decoder's: K is l x l, c = sum_i u_i row_i, phase i is decoded knowing
// u_0..u_{i-1}. With the columns of E erased and S kept, phase i is uncorrectable iff
// row_i|S lies in the span of {row_j|S : j > i}. One bottom-up elimination per pattern gives
// every phase: rows l-1 down to 0, masked by S, are inserted into an XOR basis; a row that
// reduces to zero is uncorrectable, any other joins the basis with its lowest set bit as the
// pivot. A joining row was reduced against every earlier one, so it is zero at their pivots:
// reducing in insertion order clears each pivot once and for good, and the whole elimination
// is l (l - 1) / 2 steps of (bit test, and, xor) on registers -- the loops are unrolled over
// the kernel size rounded up to 8 / 16 / 32 / 64, so the basis is never indexed by data.
//
// One lane per pattern run: a lane unranks its first combination of weight w (colex order)
// and steps with the next-same-popcount rule, or draws its patterns from Philox; the phase
// masks are summed in bit-sliced carry-save counters (kPlanes registers hold a lane's
// per-phase counts), flushed once per lane into LDS and once per workgroup into the global
// counts. No global atomics per pattern. Roofline: integer VALU only; no memory traffic
// beyond the kernel's rows (kernel arguments) and the binomial table (33 KiB, cache hits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bchk.h"
#include "bchk_env.h"
#include "bchk_philox.h"

namespace bchk {
void set_last_error(const char *msg);  // bchk_host.cpp
}

namespace {

constexpr int kBlock = 256;                        // lanes per workgroup
constexpr int kPlanes = 12;                        // carry-save planes: a lane counts < 2^12
constexpr uint32_t kRunMax = (1u << kPlanes) - 1;  // patterns per lane, at most
constexpr uint64_t kLaunchPatterns = 1ull << 28;   // patterns per launch, at most
constexpr uint64_t kTargetLanes = 1ull << 19;      // lanes a full launch is cut into (256 CUs x 2048)
constexpr int kBinomDim = 65;                      // binom[c][k], 0 <= c, k <= 64
constexpr uint32_t kDrawTag = 0xBEC00000u;         // Philox counter word 3 of a pattern draw

enum { kModeMasks = 0, kModeEnum = 1, kModeSample = 2 };

struct BecParams {
    uint64_t rows[64];           // row r of K, bit c = K[r][c]
    const uint64_t *binom;       // [kBinomDim][kBinomDim], C(c, k)
    const uint64_t *patterns;    // masks mode: the erased-column masks
    uint64_t *out;               // masks mode: masks[n]; otherwise (may be NULL) the patterns,
                                 // element first + i for the launch's i-th pattern
    unsigned long long *counts;  // [64] per-phase uncorrectable counts, added to
    uint64_t first, n;           // first rank / sample index of the launch, patterns in it
    uint64_t total;              // C(l, w): the range a sampled rank is drawn from
    uint32_t run;                // patterns per lane
    uint32_t k0, k1;             // Philox key (seed low, seed high)
    int l, w, mode;
};

int bfail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    bchk::set_last_error(buf);
    return code;
}

__device__ __forceinline__ uint32_t low_bit(uint32_t v) { return (uint32_t)__builtin_ctz(v); }
__device__ __forceinline__ uint32_t low_bit(uint64_t v) { return (uint32_t)__builtin_ctzll(v); }

// The uncorrectable phases of one erasure pattern (bit i = phase i).
template <typename W, int LP>
__device__ __forceinline__ W eliminate(const BecParams &p, uint64_t erased) {
    const W keep = (W)~erased;  // bits >= l do not matter: the rows are zero there
    W b[LP];                    // basis vector of row i (0: row i is absent or dependent)
    uint32_t pv[LP];            // its pivot column
    W unc = 0;
#pragma unroll
    for (int i = LP - 1; i >= 0; --i) {
        b[i] = 0;
        pv[i] = 0;
        if (i < p.l) {  // wave-uniform
            W v = (W)p.rows[i] & keep;
#pragma unroll
            for (int j = LP - 1; j > i; --j) v ^= b[j] & ((W)0 - ((v >> pv[j]) & (W)1));
            b[i] = v;
            pv[i] = v ? low_bit(v) : 0u;
            unc |= (W)(v == 0) << i;
        }
    }
    return unc;
}

// The combination of colex rank r among the w-subsets of {0..l-1}: its largest element is the
// largest c with C(c, w) <= r, and so on down.
__device__ inline uint64_t unrank(const uint64_t *binom, int l, int w, uint64_t r) {
    uint64_t x = 0;
    int k = w;
    for (int c = l - 1; c >= 0 && k > 0; --c) {
        const uint64_t bc = binom[c * kBinomDim + k];
        if (r >= bc) {
            x |= 1ull << c;
            r -= bc;
            --k;
        }
    }
    return x;
}

// The next larger word of the same popcount (the colex successor). x != 0, and x is not the
// last combination of a 64-bit word (the callers step only inside a lane's run).
__device__ __forceinline__ uint64_t next_combination(uint64_t x) {
    const uint64_t t = x | (x - 1);
    return (t + 1) | (((~t & (0ull - ~t)) - 1) >> (__builtin_ctzll(x) + 1));
}

// A uniform rank below total (>= 2) for sample `idx` of weight w: 64-bit candidates from the
// Philox counter (idx low, idx high, w, kDrawTag + attempt), masked to total's bit length,
// the first one below total taken. A function of (seed, w, idx) only.
__device__ inline uint64_t draw_rank(uint64_t idx, int w, uint64_t total, uint32_t k0, uint32_t k1) {
    const int bits = 64 - __builtin_clzll(total - 1);
    const uint64_t mask = bits >= 64 ? ~0ull : (1ull << bits) - 1;
    uint64_t a = 0;
    for (uint32_t attempt = 0; attempt < 64; ++attempt) {  // each fails with probability < 1/4
        const bchk::U4 r = bchk::philox(bchk::U4{(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)w, kDrawTag + attempt}, k0, k1);
        a = ((uint64_t)r.y << 32 | r.x) & mask;
        if (a < total) return a;
        a = ((uint64_t)r.w << 32 | r.z) & mask;
        if (a < total) return a;
    }
    return a % total;  // probability < 2^-128
}

template <typename W, int LP>
__global__ void __launch_bounds__(kBlock) bec_kernel(BecParams p) {
    __shared__ unsigned int wg[LP];
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t full = p.l >= 64 ? ~0ull : (1ull << p.l) - 1;
    if (p.mode == kModeMasks) {  // the whole grid takes this branch
        for (uint64_t i = t; i < p.n; i += (uint64_t)gridDim.x * kBlock)
            p.out[i] = (uint64_t)eliminate<W, LP>(p, p.patterns[i] & full);
        return;
    }
    if (threadIdx.x < LP) wg[threadIdx.x] = 0;
    __syncthreads();
    W plane[kPlanes];
#pragma unroll
    for (int q = 0; q < kPlanes; ++q) plane[q] = 0;
    uint64_t i = t * p.run;
    if (i < p.n) {
        const uint64_t end = i + p.run < p.n ? i + p.run : p.n;
        uint64_t x = p.mode == kModeEnum ? unrank(p.binom, p.l, p.w, p.first + i) : 0;
        for (; i < end; ++i) {
            if (p.mode == kModeSample)
                x = unrank(p.binom, p.l, p.w, draw_rank(p.first + i, p.w, p.total, p.k0, p.k1));
            if (p.out) p.out[p.first + i] = x;
            W carry = eliminate<W, LP>(p, x);
#pragma unroll
            for (int q = 0; q < kPlanes; ++q) {  // a lane adds at most kRunMax masks
                const W c2 = plane[q] & carry;
                plane[q] ^= carry;
                carry = c2;
            }
            if (p.mode == kModeEnum && i + 1 < end) x = next_combination(x);
        }
    }
    for (int ph = 0; ph < p.l; ++ph) {
        unsigned int v = 0;
#pragma unroll
        for (int q = 0; q < kPlanes; ++q) v |= (unsigned int)((plane[q] >> ph) & (W)1) << q;
        if (v) atomicAdd(&wg[ph], v);  // LDS, once per lane and phase
    }
    __syncthreads();
    if ((int)threadIdx.x < p.l && wg[threadIdx.x])
        atomicAdd(&p.counts[threadIdx.x], (unsigned long long)wg[threadIdx.x]);  // once per workgroup
}

void launch(const BecParams &p, unsigned blocks) {
    if (p.l <= 8)
        hipLaunchKernelGGL((bec_kernel<uint32_t, 8>), dim3(blocks), dim3(kBlock), 0, 0, p);
    else if (p.l <= 16)
        hipLaunchKernelGGL((bec_kernel<uint32_t, 16>), dim3(blocks), dim3(kBlock), 0, 0, p);
    else if (p.l <= 32)
        hipLaunchKernelGGL((bec_kernel<uint32_t, 32>), dim3(blocks), dim3(kBlock), 0, 0, p);
    else
        hipLaunchKernelGGL((bec_kernel<uint64_t, 64>), dim3(blocks), dim3(kBlock), 0, 0, p);
}

const uint64_t *binom_table() {
    static uint64_t tab[kBinomDim * kBinomDim];
    static bool done = false;
    if (!done) {  // Pascal's rule; C(64, 32) < 2^64, so nothing overflows
        for (int c = 0; c < kBinomDim; ++c)
            for (int k = 0; k < kBinomDim; ++k)
                tab[c * kBinomDim + k] = k == 0 ? 1 : (c == 0 ? 0 : tab[(c - 1) * kBinomDim + k - 1] + tab[(c - 1) * kBinomDim + k]);
        done = true;
    }
    return tab;
}

// K as row masks; BCHK_EINVAL unless 2 <= l <= max_l, entries 0/1 and K invertible.
int load_rows(const uint8_t *K, int l, int max_l, uint64_t *rows) {
    if (!K) return bfail(BCHK_EINVAL, "NULL argument");
    if (l < 2 || l > max_l) return bfail(BCHK_EINVAL, "kernel size %d unsupported (2..%d)", l, max_l);
    for (int r = 0; r < l; ++r) {
        rows[r] = 0;
        for (int c = 0; c < l; ++c) {
            if (K[r * l + c] > 1) return bfail(BCHK_EINVAL, "kernel entries must be 0 or 1");
            if (K[r * l + c]) rows[r] |= 1ull << c;
        }
    }
    std::vector<uint64_t> a(rows, rows + l);  // GF(2) rank
    for (int col = 0, r0 = 0; col < l; ++col, ++r0) {
        int piv = r0;
        while (piv < l && !((a[piv] >> col) & 1ull)) ++piv;
        if (piv == l) return bfail(BCHK_EINVAL, "kernel is singular");
        std::swap(a[piv], a[r0]);
        for (int r = 0; r < l; ++r)
            if (r != r0 && ((a[r] >> col) & 1ull)) a[r] ^= a[r0];
    }
    return BCHK_OK;
}

// Device scratch of one call: the binomial table, the per-phase counts, the pattern buffer.
struct BecScratch {
    uint64_t *binom = nullptr;
    unsigned long long *counts = nullptr;
    uint64_t *pat = nullptr;
    ~BecScratch() {
        if (binom) (void)hipFree(binom);
        if (counts) (void)hipFree(counts);
        if (pat) (void)hipFree(pat);
    }
    int init(int device) {
        if (hipSetDevice(device) != hipSuccess) return bfail(BCHK_ENODEV, "hipSetDevice(%d) failed", device);
        const size_t tb = sizeof(uint64_t) * kBinomDim * kBinomDim;
        if (hipMalloc((void **)&binom, tb) != hipSuccess || hipMalloc((void **)&counts, 64 * sizeof(unsigned long long)) != hipSuccess)
            return bfail(BCHK_ENOMEM, "hipMalloc failed");
        if (hipMemcpy(binom, binom_table(), tb, hipMemcpyHostToDevice) != hipSuccess)
            return bfail(BCHK_EHIP, "hipMemcpy of the binomial table failed");
        return BCHK_OK;
    }
};

// patterns per lane: BCHK_BEC_RUN in the environment (1..kRunMax), else sized so that a full
// launch is about kTargetLanes lanes. Counts do not depend on it.
uint32_t pick_run(uint64_t n) {
    int v = 0;
    if (bchk::env_int("BCHK_BEC_RUN", &v, 0, (int)kRunMax) && v >= 1) return (uint32_t)v;
    const uint64_t r = (n + kTargetLanes - 1) / kTargetLanes;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(r, 1), kRunMax);
}

// All `count` patterns of one weight (ranks or sample indices 0..count-1), in launches of at
// most kLaunchPatterns; out[phase] = the uncorrectable counts. p carries rows, l, w, mode,
// total, key and (pre-set) out.
int run_weight(BecParams p, BecScratch &s, uint64_t count, uint64_t *out) {
    if (hipMemset(s.counts, 0, 64 * sizeof(unsigned long long)) != hipSuccess) return bfail(BCHK_EHIP, "hipMemset failed");
    p.binom = s.binom;
    p.counts = s.counts;
    for (uint64_t first = 0; first < count; first += kLaunchPatterns) {
        p.first = first;
        p.n = std::min(kLaunchPatterns, count - first);
        p.run = pick_run(p.n);
        const uint64_t lanes = (p.n + p.run - 1) / p.run;
        launch(p, (unsigned)((lanes + kBlock - 1) / kBlock));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return bfail(BCHK_EHIP, "bec_kernel launch: %s", hipGetErrorString(e));
    }
    unsigned long long h[64];
    const hipError_t e = hipMemcpy(h, s.counts, sizeof h, hipMemcpyDeviceToHost);  // waits for the launches
    if (e != hipSuccess) return bfail(BCHK_EHIP, "bec_kernel: %s", hipGetErrorString(e));
    for (int i = 0; i < p.l; ++i) out[i] = h[i];
    return BCHK_OK;
}

}  // namespace

extern "C" {

int bchk_kernel_bec_masks(const uint8_t *K, int l, const uint64_t *patterns, size_t n, int device, uint64_t *masks) {
    BecParams p{};
    if (int rc = load_rows(K, l, 64, p.rows)) return rc;
    if (n && (!patterns || !masks)) return bfail(BCHK_EINVAL, "NULL argument");
    if (n == 0) return BCHK_OK;
    if (hipSetDevice(device) != hipSuccess) return bfail(BCHK_ENODEV, "hipSetDevice(%d) failed", device);
    uint64_t *d = nullptr;
    if (hipMalloc((void **)&d, 2 * n * sizeof(uint64_t)) != hipSuccess) return bfail(BCHK_ENOMEM, "hipMalloc(%zu) failed", 2 * n * sizeof(uint64_t));
    hipError_t e = hipMemcpy(d, patterns, n * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        p.patterns = d;
        p.out = d + n;
        p.n = n;
        p.l = l;
        p.mode = kModeMasks;
        const uint64_t blocks = std::min<uint64_t>((n + kBlock - 1) / kBlock, 8192);  // grid-stride beyond
        launch(p, (unsigned)blocks);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(masks, d + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return bfail(BCHK_EHIP, "bec_kernel (masks): %s", hipGetErrorString(e));
    return BCHK_OK;
}

int bchk_kernel_bec_behaviour(const uint8_t *K, int l, int w_lo, int w_hi, int device, uint64_t *counts) {
    BecParams p{};
    if (int rc = load_rows(K, l, 32, p.rows)) return rc;
    if (!counts) return bfail(BCHK_EINVAL, "NULL argument");
    if (w_lo < 0 || w_hi > l || w_lo > w_hi) return bfail(BCHK_EINVAL, "weights %d..%d outside 0..%d", w_lo, w_hi, l);
    std::memset(counts, 0, sizeof(uint64_t) * (size_t)l * (l + 1));
    BecScratch s;
    if (int rc = s.init(device)) return rc;
    p.l = l;
    p.mode = kModeEnum;
    for (int w = w_lo; w <= w_hi; ++w) {
        uint64_t col[64];
        p.w = w;
        p.total = binom_table()[l * kBinomDim + w];
        if (int rc = run_weight(p, s, p.total, col)) return rc;
        for (int i = 0; i < l; ++i) counts[(size_t)i * (l + 1) + w] = col[i];
    }
    return BCHK_OK;
}

int bchk_kernel_bec_sample(const uint8_t *K, int l, uint64_t samples, uint64_t seed, int device, uint64_t *unc,
                           uint64_t *tried, uint8_t *exact, int pattern_weight, uint64_t *patterns) {
    BecParams p{};
    if (int rc = load_rows(K, l, 64, p.rows)) return rc;
    if (!unc || !tried || !exact) return bfail(BCHK_EINVAL, "NULL argument");
    if (samples < 1 || samples > (1ull << 40)) return bfail(BCHK_EINVAL, "samples must be 1..2^40");
    if (patterns && (pattern_weight < 0 || pattern_weight > l)) return bfail(BCHK_EINVAL, "pattern weight %d outside 0..%d", pattern_weight, l);
    std::memset(unc, 0, sizeof(uint64_t) * (size_t)l * (l + 1));
    BecScratch s;
    if (int rc = s.init(device)) return rc;
    p.l = l;
    p.k0 = (uint32_t)seed;
    p.k1 = (uint32_t)(seed >> 32);
    for (int w = 0; w <= l; ++w) {
        uint64_t col[64];
        p.w = w;
        p.total = binom_table()[l * kBinomDim + w];
        const bool ex = p.total <= samples;
        const uint64_t count = ex ? p.total : samples;
        p.mode = ex ? kModeEnum : kModeSample;
        p.out = nullptr;
        const bool keep = patterns && w == pattern_weight;
        if (keep) {
            if (hipMalloc((void **)&s.pat, count * sizeof(uint64_t)) != hipSuccess) return bfail(BCHK_ENOMEM, "hipMalloc(%llu) failed", (unsigned long long)(count * sizeof(uint64_t)));
            p.out = s.pat;
        }
        if (int rc = run_weight(p, s, count, col)) return rc;
        if (keep && hipMemcpy(patterns, s.pat, count * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
            return bfail(BCHK_EHIP, "hipMemcpy of the patterns failed");
        for (int i = 0; i < l; ++i) unc[(size_t)i * (l + 1) + w] = col[i];
        tried[w] = count;
        exact[w] = ex ? 1 : 0;
    }
    return BCHK_OK;
}

}  // extern "C"
