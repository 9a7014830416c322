// polar_host.cpp -- host runtime of the GPU SC-list decoder behind the C ABI (bchk_polar_*
// in include/bchk.h): the reference's code specification, the dynamic-freezing masks, the
// device tables and the batched launch. Replaces CMixedKernelListDecoder(Spec, ListSize)
// and Decode(pLLR, pInfVectorList, pCodewordList) (headers/external/MixedKernelListDecoder.h:
// 27-39, out/external/MixedKernelListDecoder.cpp:9, :211-268) and CMixedKernelEncoder::Encode
// (out/external/MixedKernelEncoder.cpp:142-177). All decoding runs on the GPU. Also the
// simulation front-end (polar_channel.hip): encode, words over AWGN, Rayleigh fading or the BSC,
// the simulator's counters and the sweep of CSimulator (out/external/Simulator.cpp:104-114,
// :139-335, channels :179-191), and the
// genie-aided SC runs (polar_genie.hip) behind bchk_polar_genie_device / bchk_polar_genie_run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cfloat>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "bchk.h"
#include "bchk_env.h"
#include "polar_device.h"

using namespace bchk;

namespace bchk {
hipError_t launch_polar(const PolarParams &p, int grid, size_t lds, hipStream_t s);
const void *polar_kernel_ptr();
hipError_t launch_polar_tiered(const PolarTieredParams &p, int grid, size_t lds, hipStream_t s);  // polar_sclist_tiered.hip
const void *polar_tiered_kernel_ptr();
hipError_t launch_polar_mixed(const PolarMixedParams &p, int grid, size_t lds, hipStream_t s);
const void *polar_mixed_kernel_ptr();
hipError_t launch_polar_mixed_tiered(const PolarMixedTieredParams &p, int grid, size_t lds, hipStream_t s);  // polar_mixed_tiered.hip
const void *polar_mixed_tiered_kernel_ptr();
hipError_t launch_polar_q8(const PolarQ8Params &p, int grid, size_t lds, hipStream_t s);  // polar_sclist_q8.hip
const void *polar_q8_kernel_ptr();
hipError_t launch_polar_q8_tiered(const PolarQ8TieredParams &p, int grid, size_t lds, hipStream_t s);  // polar_sclist_q8_tiered.hip
const void *polar_q8_tiered_kernel_ptr();
hipError_t launch_polar_quantize(const float *llr, size_t count, float scale, int qmax, int8_t *q, hipStream_t s);
hipError_t launch_polar_gen(const PolarGenParams &p, hipStream_t s);      // polar_channel.hip
hipError_t launch_polar_count(const PolarCountParams &p, hipStream_t s);
hipError_t launch_polar_genie(const PolarGenieParams &p, int grid, size_t lds, hipStream_t s);  // polar_genie.hip
hipError_t launch_polar_genie_sum(const float *dec_llr, const uint8_t *u, uint32_t B, int U, uint64_t *err,
                                  int64_t *soft, hipStream_t s);
const void *polar_genie_kernel_ptr();
void set_last_error(const char *msg);  // bchk_host.cpp: the message bchk_last_error returns
int polar_check_channel(int channel, double param);  // below; polar_design.cpp calls both too
int polar_check_fading(int kind, double param);
}  // namespace bchk

namespace {

int pfail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_last_error(buf);
    return code;
}

#define PHIP_TRY(expr)                                                                  \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return pfail(BCHK_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                         __FILE__, __LINE__);                                           \
    } while (0)

struct PBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) return pfail(BCHK_ENOMEM, "hipMalloc(%zu) failed", bytes);
        cap = bytes;
        return 0;
    }
    PBuf() = default;
    PBuf(const PBuf &) = delete;
    PBuf &operator=(const PBuf &) = delete;
    ~PBuf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

struct bchk_polar {
    enum class PolarState { List, Mixed, ListTiered, MixedTiered, ListQ8, ListQ8Tiered };
    int N = 0, K = 0, U = 0, n = 0, L = 0, device = 0;
    // layers: kernel size, Arikan flag, rows as bitmasks (bit c = K[r][c]); mixed = any
    // matrix or named (G / A5) layer (decoded by polar_mixed_kernel)
    bool mixed = false;
    std::vector<int> ksize;
    std::vector<uint8_t> arikan;
    std::vector<uint8_t> named;   // kNamedG / kNamedA5 (polar_device.h), 0 otherwise
    std::vector<uint64_t> krows;  // [layer][kPolarMaxKernel]
    PolarMixedParams mp{};        // the mixed layout (sizes, offsets)
    size_t off_krows = 0;
    std::vector<uint32_t> tent, tbase;  // matrix-layer trellises (polar_device.h)
    std::vector<uint8_t> tlog;
    size_t off_tent = 0, off_tbase = 0, off_tlog = 0;
    std::vector<int16_t> symmap, infopos, cwpos;
    std::vector<uint8_t> frozen;
    std::vector<int8_t> dfbit;
    std::vector<uint64_t> dfcorr;
    std::vector<std::vector<int>> fc;  // freezing constraints (terms, frozen symbol last)
    std::vector<int> decision;         // constraint of each symbol, -1 = unfrozen
    uint8_t *d_tab = nullptr;          // one blob: symmap | phase | cwpos | dfcorr | ... | encoder tables
    size_t off_symmap = 0, off_phase = 0, off_cwpos = 0, off_dfcorr = 0;
    // the device encoder's tables (polar_device.h PolarEncTables)
    std::vector<int16_t> inforank;
    std::vector<uint32_t> dynoff;
    std::vector<uint16_t> dynterm;
    size_t off_inforank = 0, off_dynoff = 0, off_dynterm = 0;
    hipStream_t stream = nullptr;
    size_t lds = 0;
    int grid = 0;
    PBuf llr, info, cw, metric, count;
    PBuf txinfo, txcw, flags, cnt8;  // bchk_polar_sweep_device's sent words, error flags, counters
    PBuf q8;                         // bchk_polar_sweep_q8_device's quantised LLRs
    // time-budgeted launches of codes with search layers (PolarMixedParams::budget)
    PBuf rstate, rsave, unfinished;
    uint64_t budget_ticks = 0;  // 100 MHz ticks per launch, 0 = one launch per call
    uint64_t launches_last = 0; // launches the last budgeted call took
    // genie-aided SC (polar_genie.hip): the one-path layout, set up by the first genie call
    PolarGenieParams gp{};
    size_t genie_lds = 0;
    int genie_grid = 0;
    PBuf gdec, gu, gsum;  // decision-LLR and u rows when the caller passes none; bchk_polar_genie_run's counters
    // Where the path state lives, and so which kernel decodes. ListTiered
    // (polar_sclist_tiered.hip): layers 1..split and C_0 of every path in `ws`. MixedTiered
    // (polar_mixed_tiered.hip): the groups of the layers j < split in `ws`; tm.m holds the tiered
    // layout, mp stays the LDS layout (the genie calls use it). ListQ8 (polar_sclist_q8.hip): List
    // with int8 LLRs, decoded through bchk_polar_decode_q8_* only. ListQ8Tiered
    // (polar_sclist_q8_tiered.hip): ListTiered with int8 LLRs, through the same calls.
    PolarState state = PolarState::List;
    int split = 0, cwsplit = 0, cwall = 0;
    PBuf ws;  // [grid] workspaces of ws_bytes(c) each
    PolarMixedTieredParams tm{};
    bool is_tiered() const {
        return state == PolarState::ListTiered || state == PolarState::MixedTiered || state == PolarState::ListQ8Tiered;
    }
    bool is_q8() const { return state == PolarState::ListQ8 || state == PolarState::ListQ8Tiered; }  // an int8 context
};
using State = bchk_polar::PolarState;

namespace {

constexpr size_t kPolarLdsMax = 160 * 1024;

// the tiered kernels' LDS and workspace layout at `split` (polar_device.h), f32 or int8 LLRs
PolarTieredLayout tiered_layout(const bchk_polar *c, int split, bool q8 = false) {
    int32_t off[kPolarMaxLayers + 1];
    (void)polar_cw_layout(c->U, off);
    const int words = off[c->n] + 1;  // C_n is one word
    const int cwsplit = split < c->n ? off[split + 1] : words;
    return q8 ? polar_q8_tiered_layout(c->U, c->L, c->K, split, cwsplit, words)
              : polar_tiered_layout(c->U, c->L, c->K, split, cwsplit, words);
}
// Waves per CU that LDS allows, up to kTieredWaves: past that the decoder is bound by the
// latency of its global layers, not by the waves in flight.
constexpr int kTieredWaves = 8;
int tiered_waves(size_t lds) { return (int)std::min<size_t>(kTieredWaves, kPolarLdsMax / std::max<size_t>(lds, 1)); }

// the mixed kernel's LDS and save-slot layout (polar_device.h)
PolarMixedLayout mixed_lds(const bchk_polar *c) {
    const PolarMixedParams &m = c->mp;
    return polar_mixed_layout(c->U, c->L, c->K, m.ssize, m.csize, m.osize, m.nl, m.tstates, m.any_ml != 0);
}

// The specification (MixedKernelEncoder.cpp:7-98): header, kernel names, shortened and
// punctured symbols, then U - K freezing constraints "w t_1 ... t_w" (ascending, the frozen
// symbol last).
// GetKernelByName (Kernel.cpp:235-274): "A", "G" or "A5" (any case, _stricmp), or a matrix
// file "-path" / "<path" (relative to kdir) holding the size and size^2 entries
// (Kernel.cpp:93-107); the kernel must be invertible (Kernel.cpp:155-176). *named: kNamedG /
// kNamedA5 for the kernels of TruncatedArikanKernel.cpp, decoded by their own f/g processors.
// Their rows are what CGKernel::Multiply (:18-30) and CA5Kernel::Multiply (:204-216) compute,
// which is what the library encodes and decodes with. For A5 that is the matrix of the
// file's comment (:193-197), rows 10000 / 11000 / 10100 / 10001 / 11110; the A5[] array
// GetKernel() returns (:251-258) has the last two rows the other way round and is not used.
int read_kernel(const std::string &name, const char *kdir, int *size, uint64_t *rows, bool *arikan, uint8_t *named) {
    std::string low = name;
    for (char &ch : low) ch = (char)tolower((unsigned char)ch);
    *named = 0;
    if (low == "a") {
        *size = 2;
        rows[0] = 1u;       // 1 0
        rows[1] = 3u;       // 1 1  (Kernel.cpp:8-12)
        *arikan = true;
        return 0;
    }
    if (low == "g" || low == "a5") {
        static const uint64_t g3[3] = {1u, 3u, 6u}, a5[5] = {1u, 3u, 5u, 17u, 15u};  // bit c = K[r][c]
        *size = low == "g" ? 3 : 5;
        for (int r = 0; r < *size; ++r) rows[r] = low == "g" ? g3[r] : a5[r];
        *arikan = false;
        *named = low == "g" ? kNamedG : kNamedA5;
        return 0;
    }
    if (name.empty() || (name[0] != '-' && name[0] != '<')) return pfail(BCHK_EINVAL, "Unknown kernel %s", name.c_str());
    std::string path = name.substr(1);
    if (!path.empty() && path[0] != '/' && kdir && kdir[0]) path = std::string(kdir) + "/" + path;
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return pfail(BCHK_EINVAL, "Error reading kernel file %s", path.c_str());
    int l = 0;
    if (fscanf(f, "%d", &l) != 1 || l < 2 || l > kPolarMaxKernel) {
        fclose(f);
        return pfail(BCHK_EINVAL, "Error reading kernel file %s (size)", path.c_str());
    }
    for (int r = 0; r < l; ++r) {
        rows[r] = 0;
        for (int q = 0; q < l; ++q) {
            unsigned v;
            if (fscanf(f, "%u", &v) != 1) {
                fclose(f);
                return pfail(BCHK_EINVAL, "Error parsing kernel file %s", path.c_str());
            }
            if (v) rows[r] |= 1ull << q;
        }
    }
    fclose(f);
    std::vector<uint64_t> a(rows, rows + l);  // GF(2) rank
    for (int col = 0, r0 = 0; col < l; ++col) {
        int piv = r0;
        while (piv < l && !((a[piv] >> col) & 1ull)) ++piv;
        if (piv == l) return pfail(BCHK_EINVAL, "Kernel is singular (%s)", path.c_str());
        std::swap(a[piv], a[r0]);
        for (int r = 0; r < l; ++r)
            if (r != r0 && ((a[r] >> col) & 1ull)) a[r] ^= a[r0];
        ++r0;
    }
    if (l > kPolarMaxMatrixGpu)
        return pfail(BCHK_EINVAL, "matrix kernel of size %d: the GPU SC-list decoder takes sizes up to %d", l,
                     kPolarMaxMatrixGpu);
    *size = l;
    *arikan = false;
    return 0;
}

// CTrellisKernelProcessor's trellis of every phase of an l x l kernel (out/external/
// TrellisKernelProcessor.cpp:69-179: MinimumSpan :7-67 of rows phase..l-1 with row `phase`
// extended by a 1 at position l, states = active rows, state bits compressed as rows end),
// stored as predecessor lists for the GPU's pull-form Viterbi (polar_device.h). Appends to
// ent; base[phase], lg[phase * (kPolarMaxKernel + 1) + d]; returns the largest state count
// (0 and a message when a depth needs more than 2^kPolarTrellisMaxBits states).
int build_trellis(const uint64_t *rows, int l, std::vector<uint32_t> &ent, uint32_t *base, uint8_t *lg) {
    if (l > kPolarMaxTrellisKernel) return pfail(BCHK_EINVAL, "no trellis for a kernel of size %d (> %d)", l, kPolarMaxTrellisKernel), 0;
    int most = 1;
    const unsigned N = (unsigned)l + 1u;
    for (int ph = 0; ph < l; ++ph) {
        const unsigned K = (unsigned)(l - ph);
        uint64_t M[kPolarMaxKernel];
        for (unsigned i = 0; i < K; ++i) M[i] = rows[ph + (int)i];
        M[0] |= 1ull << l;
        unsigned start[kPolarMaxKernel + 1], end[kPolarMaxKernel + 1];
        for (unsigned c = 0; c < N; ++c) start[c] = end[c] = ~0u;
        unsigned C = 0;  // MinimumSpan (:7-67)
        for (unsigned i = 0; i < K; ++i) {
            bool found = false;
            for (; C < N; ++C) {
                if (!((M[i] >> C) & 1ull)) {
                    for (unsigned j = i + 1; j < K; ++j)
                        if ((M[j] >> C) & 1ull) {
                            M[i] ^= M[j];
                            found = true;
                            break;
                        }
                    if (found) {
                        start[C] = i;
                        break;
                    }
                } else {
                    start[C] = i;
                    found = true;
                    break;
                }
            }
            if (!found) return pfail(BCHK_EINVAL, "Matrix is not full rank"), 0;
            for (unsigned j = i + 1; j < K; ++j)
                if ((M[j] >> C) & 1ull) M[j] ^= M[i];
        }
        for (int i = (int)K - 1; i >= 0; --i)
            for (int j = (int)N - 1; j >= 0; --j)
                if ((M[i] >> j) & 1ull) {
                    end[j] = (unsigned)i;
                    for (int q = 0; q < i; ++q)
                        if ((M[q] >> j) & 1ull) M[q] ^= M[i];
                    break;
                }
        base[ph] = (uint32_t)ent.size();
        uint8_t *lgp = lg + (size_t)ph * (kPolarMaxKernel + 1);
        lgp[0] = 0;
        std::vector<uint64_t> cw0(1, 0ull), cw1;
        unsigned active[kPolarMaxKernel + 1], na = 0;
        for (int j = 0; j < l; ++j) {  // :107-158, depths 0..l-1 (GetLLRs never reads depth l's edges)
            unsigned B = na;
            for (unsigned q = 0; q < na; ++q)
                if (active[q] == end[j]) { B = q; break; }
            const uint64_t emask = (end[j] == ~0u) ? ~0ull : ((1ull << B) - 1ull);
            const uint64_t ns = 1ull << na;
            const unsigned na1 = na + (start[j] != ~0u ? 1u : 0u) - (end[j] != ~0u ? 1u : 0u);
            if (na1 > (unsigned)kPolarTrellisMaxBits || na + 1 > (unsigned)kPolarTrellisMaxBits + 1)
                return pfail(BCHK_EINVAL, "kernel of size %d: its trellis needs 2^%u states (GPU limit 2^%d)", l,
                             std::max(na1, na), kPolarTrellisMaxBits), 0;
            const uint64_t ns1 = 1ull << na1;
            cw1.assign(ns1, 0ull);
            const size_t e0 = ent.size();
            ent.resize(e0 + ns1, 0u);
            auto link = [&](uint64_t S, uint64_t S1, uint32_t z) {
                uint32_t &e = ent[e0 + S1];
                const uint32_t h = (uint32_t)S | (z ? kTrellisZ : 0u) | kTrellisValid;
                if (!(e & kTrellisValid)) e |= h;
                else e |= h << 16;
            };
            if (start[j] == ~0u) {
                for (uint64_t S = 0; S < ns; ++S) {
                    const uint32_t bit = (uint32_t)((cw0[S] >> j) & 1ull);
                    const uint64_t nx = (S & emask) | ((S >> 1) & ~emask);
                    cw1[nx] = cw0[S];
                    link(S, nx, bit);
                }
            } else {
                for (uint64_t S = 0; S < ns; ++S) {
                    uint64_t n0 = S, n1 = S ^ (1ull << na);
                    n0 = (n0 & emask) | ((n0 >> 1) & ~emask);
                    n1 = (n1 & emask) | ((n1 >> 1) & ~emask);
                    const uint64_t c1 = cw0[S] ^ M[start[j]];
                    cw1[n0] = cw0[S];
                    cw1[n1] = c1;
                    link(S, n0, (uint32_t)((cw0[S] >> j) & 1ull));
                    link(S, n1, (uint32_t)((c1 >> j) & 1ull));
                }
                active[na++] = start[j];
            }
            cw0.swap(cw1);
            if (end[j] != ~0u) {
                memmove(active + B, active + B + 1, sizeof(unsigned) * (na - B - 1));
                --na;
            }
            if (na != na1) return pfail(BCHK_EINVAL, "trellis construction inconsistent"), 0;
            lgp[j + 1] = (uint8_t)na;
            most = std::max(most, 1 << na);
        }
    }
    return most;
}

int parse_spec(bchk_polar *c, const char *spec, const char *kdir) {
    std::istringstream in(spec);
    int N, K, dmin, layers, nsh, npu;
    if (!(in >> N >> K >> dmin >> layers >> nsh >> npu)) return pfail(BCHK_EINVAL, "Error reading file header");
    if (K > N || K < 0 || N <= 0) return pfail(BCHK_EINVAL, "Code dimension cannot exceed code length");
    if (layers < 1 || layers > kPolarMaxLayers) return pfail(BCHK_EINVAL, "%d layers unsupported", layers);
    c->ksize.assign(layers, 2);
    c->arikan.assign(layers, 1);
    c->named.assign(layers, 0);
    c->krows.assign((size_t)layers * kPolarMaxKernel, 0ull);
    long Ul = 1;
    for (int i = 0; i < layers; ++i) {
        std::string name;
        if (!(in >> name)) return pfail(BCHK_EINVAL, "missing kernel name %d", i);
        bool ar = false;
        if (int rc = read_kernel(name, kdir, &c->ksize[i], &c->krows[(size_t)i * kPolarMaxKernel], &ar,
                                 &c->named[i]))
            return rc;
        c->arikan[i] = ar ? 1 : 0;
        c->mixed = c->mixed || !ar;
        Ul *= c->ksize[i];
        if (Ul > 16384) return pfail(BCHK_EINVAL, "length %ld exceeds 16384", Ul);
    }
    const int U = (int)Ul;
    if (N + nsh + npu != U) return pfail(BCHK_EINVAL, "Code length mismatch");
    c->N = N;
    c->K = K;
    c->U = U;
    c->n = layers;
    std::vector<uint8_t> type(U, 0);
    for (int i = 0; i < nsh + npu; ++i) {
        int s;
        if (!(in >> s) || s < 0 || s >= U) return pfail(BCHK_EINVAL, "Invalid shortened / punctured symbol");
        type[s] = (uint8_t)(i < nsh ? 1 : 2);
    }
    c->decision.assign(U, -1);
    c->fc.assign(U - K, {});
    for (int i = 0; i < U - K; ++i) {
        int w;
        if (!(in >> w) || w < 1) return pfail(BCHK_EINVAL, "Error reading freezing constraint %d", i);
        for (int j = 0; j < w; ++j) {
            int v;
            if (!(in >> v) || v < 0 || v >= U || (j && v <= c->fc[i].back()))
                return pfail(BCHK_EINVAL, "Invalid freezing constraint %d", i);
            c->fc[i].push_back(v);
        }
        const int last = c->fc[i].back();
        if (c->decision[last] != -1) return pfail(BCHK_EINVAL, "Duplicate freezing constraint on symbol %d", last);
        c->decision[last] = i;
    }
    // dynamic-freezing value bits (KernelListEngine.cpp:6-39)
    c->dfbit.assign(U, -1);
    c->dfcorr.assign(U, 0);
    uint64_t avail = ~0ull;
    for (int i = 0; i < U; ++i) {
        if (c->dfbit[i] >= 0) avail |= 1ull << c->dfbit[i];
        for (int j = i + 1; j < U; ++j) {
            const int ci = c->decision[j];
            if (ci < 0 || c->fc[ci][0] != i) continue;
            if (!avail) return pfail(BCHK_EINVAL, "Too many dynamic freezing constraints are simultaneously active");
            const int B = __builtin_ctzll(avail);
            avail &= ~(1ull << B);
            c->dfbit[j] = (int8_t)B;
            for (int t : c->fc[ci]) {
                if (t == j) break;
                c->dfcorr[t] ^= 1ull << B;
            }
            c->dfcorr[j] ^= 1ull << B;
        }
    }
    c->symmap.assign(U, 0);
    c->frozen.assign(U, 0);
    c->infopos.clear();
    c->cwpos.clear();
    for (int i = 0, I = 0; i < U; ++i) {
        c->symmap[i] = (int16_t)(type[i] == 0 ? I++ : (type[i] == 1 ? -1 : -2));
        if (type[i] == 0) c->cwpos.push_back((int16_t)i);
        c->frozen[i] = c->decision[i] >= 0;
        if (c->decision[i] < 0) c->infopos.push_back((int16_t)i);
    }
    // the device encoder: where each information bit goes, and the dynamic constraints (more
    // than one term) in the order of their frozen symbols
    c->inforank.assign(U, -1);
    c->dynoff.assign(1, 0u);
    c->dynterm.clear();
    for (int i = 0, k = 0; i < U; ++i) {
        const int ci = c->decision[i];
        if (ci < 0) {
            c->inforank[i] = (int16_t)k++;
        } else if (c->fc[ci].size() > 1) {
            for (int t : c->fc[ci]) c->dynterm.push_back((uint16_t)t);
            c->dynoff.push_back((uint32_t)c->dynterm.size());
        }
    }
    return 0;
}

// the mixed layout of one path (oracle/polar_oracle.c plr_decode's offsets). A named layer
// (G / A5) has no offset state; its processor's float state follows the S layers in the path's
// S stride and A5's bit takes the layer's place in the offset-state stride (polar_device.h).
// With such a layer the S stride gets polar_path_s's 16 bytes of padding: the state is read
// and written at stride d across the lanes, like S, one path after the other.
// The strides and offsets of the layers from `first` on (S_{first+1} .. and C_{first+1} ..,
// counted from 0) are what both layouts share.
void inner_layout(const bchk_polar *c, int first, PolarMixedParams &m) {
    const int nl = c->n;
    int so = 0, co = first ? 0 : m.outer[0], oo = 0;  // C_0 leads the path's C stride when it is in LDS
    for (int lam = first + 1; lam <= nl; ++lam) { m.soff[lam] = so; so += m.outer[lam]; }
    for (int lam = first + 1; lam <= nl; ++lam) { m.coff[lam] = co; co += m.outer[lam] * c->ksize[lam - 1]; }
    bool any_named = false;
    for (int j = first; j < nl; ++j) {
        m.ooff[j] = oo;
        m.foff[j] = so;
        if (c->named[j]) {
            any_named = true;
            so += polar_named_floats(c->named[j]) * m.outer[j + 1];
            if (c->named[j] == kNamedA5) oo += m.outer[j + 1];
        } else if (!c->arikan[j]) {
            oo += c->ksize[j] * m.outer[j + 1];
        }
    }
    m.ssize = (so || !first) ? ((so + 3) & ~3) + (any_named ? 4 : 0) : 0;
    m.csize = (co + 15) & ~15;
    m.osize = (oo + 15) & ~15;
}
void mixed_layout(const bchk_polar *c, PolarMixedParams &m) {
    const int nl = c->n;
    m.nl = nl;
    m.outer[0] = c->U;
    for (int j = 0; j < nl; ++j) {
        m.ksize[j] = c->ksize[j];
        m.arikan[j] = c->arikan[j];
        m.named[j] = c->named[j];
        m.outer[j + 1] = m.outer[j] / c->ksize[j];
    }
    m.soff[0] = 0;
    m.coff[0] = 0;
    inner_layout(c, 0, m);
}

// The mixed layout of a context and how each matrix layer takes its LLRs, with the trellises
// (c->mp, c->tent / tbase / tlog).
int mixed_tables(bchk_polar *c) {
    PolarMixedParams &m = c->mp;
    const int nl = c->n;
    mixed_layout(c, m);
    // matrix layers from the trellis threshold up take their LLRs from the trellis; those
    // larger than the trellis limit (or from BCHK_POLAR_ML up) from the exact
    // ordered-statistics search
    int tmin = 16, mlmin = kPolarMaxTrellisKernel + 1;
    env_int("BCHK_POLAR_TRELLIS", &tmin, 2, INT_MAX);
    env_int("BCHK_POLAR_ML", &mlmin, 2, INT_MAX);
    // the search's round guard (a finite tree: never reached in practice; tests lower it)
    int rounds = 0;
    m.ml_rounds = env_int("BCHK_POLAR_ML_ROUNDS", &rounds, 1, INT_MAX) ? (uint32_t)rounds : kMlRoundsDefault;
    m.any_ml = 0;
    m.tstates = 0;
    c->tbase.assign((size_t)nl * kPolarMaxKernel, 0u);
    c->tlog.assign((size_t)nl * kPolarMaxKernel * (kPolarMaxKernel + 1), 0u);
    c->tent.clear();
    for (int j = 0; j < nl; ++j) {
        const bool matrix = !c->arikan[j] && !c->named[j];  // LLRs over the coset of its rows
        m.ml[j] = (matrix && c->ksize[j] >= std::min(mlmin, kPolarMaxTrellisKernel + 1)) ? 1 : 0;
        m.any_ml |= m.ml[j];
        m.trellis[j] = (matrix && !m.ml[j] && c->ksize[j] >= tmin) ? 1 : 0;
        if (!m.trellis[j]) continue;
        const int most = build_trellis(&c->krows[(size_t)j * kPolarMaxKernel], c->ksize[j], c->tent,
                                       &c->tbase[(size_t)j * kPolarMaxKernel],
                                       &c->tlog[(size_t)j * kPolarMaxKernel * (kPolarMaxKernel + 1)]);
        if (!most) return BCHK_EINVAL;  // build_trellis set the message
        m.tstates = std::max(m.tstates, std::max(64, most));
    }
    if (c->tent.empty()) c->tent.push_back(0u);
    return 0;
}

// The tiered mixed layout at `split` (polar_device.h PolarMixedTieredParams): the LDS strides
// and offsets of the inner layers j >= split in mixed_layout's form, and for j < split the parts
// of one array of the layer's group (S, F, then C and O on 16 bytes).
void mixed_tiered_layout(const bchk_polar *c, int split, PolarMixedTieredParams &t) {
    PolarMixedParams &m = t.m;
    m = c->mp;
    t.split = split;
    int grp = 0;
    for (int j = 0; j < split; ++j) {
        const int d = m.outer[j + 1], l = c->ksize[j];
        const bool matrix = !c->arikan[j] && !c->named[j];
        t.gfloats[j] = polar_named_floats(c->named[j]) * d;
        t.gobytes[j] = matrix ? l * d : (c->named[j] == kNamedA5 ? d : 0);
        m.soff[j + 1] = 0;
        m.foff[j] = d;
        m.coff[j + 1] = (4 * (d + t.gfloats[j]) + 15) & ~15;
        m.ooff[j] = (m.coff[j + 1] + l * d + 15) & ~15;
        t.garr[j] = (m.ooff[j] + t.gobytes[j] + 15) & ~15;
        t.gbase[j] = grp;
        grp += c->L * t.garr[j];
    }
    t.grp_bytes = grp;
    m.coff[0] = 0;
    inner_layout(c, split, m);
}
PolarMixedTieredLayout mixed_tiered_lds(const bchk_polar *c, const PolarMixedTieredParams &t) {
    const PolarMixedParams &m = t.m;
    return polar_mixed_tiered_layout(c->U, c->L, c->K, m.ssize, m.csize, m.osize, m.nl, t.split, m.tstates, t.grp_bytes);
}
size_t mixed_tiered_lds_at(const bchk_polar *c, int split) {
    PolarMixedTieredParams t{};
    mixed_tiered_layout(c, split, t);
    return mixed_tiered_lds(c, t).bytes;
}

// a workgroup's workspace in the state's layout (0: every path's state in LDS)
uint64_t ws_bytes(const bchk_polar *c) {
    switch (c->state) {
    case State::ListTiered: return tiered_layout(c, c->split).ws_bytes;
    case State::ListQ8Tiered: return tiered_layout(c, c->split, true).ws_bytes;
    case State::MixedTiered: return mixed_tiered_lds(c, c->tm).ws_bytes;
    default: return 0;
    }
}
// The split a tiered state chooses (counting layers from the channel side; lds_at(s): LDS bytes
// at split s): the smallest whose LDS part fits, then further layers out while that lets one
// more wave onto a CU (tiered_waves).
template <class LdsAt>
int auto_split(const bchk_polar *c, LdsAt lds_at) {
    int s = 1;
    while (s < c->n && lds_at(s) > kPolarLdsMax) ++s;
    while (s < c->n && tiered_waves(lds_at(s + 1)) > tiered_waves(lds_at(s))) ++s;
    return s;
}
// the state's kernel
const void *kernel_ptr(State st) {
    switch (st) {
    case State::List: return polar_kernel_ptr();
    case State::Mixed: return polar_mixed_kernel_ptr();
    case State::ListTiered: return polar_tiered_kernel_ptr();
    case State::MixedTiered: return polar_mixed_tiered_kernel_ptr();
    case State::ListQ8: return polar_q8_kernel_ptr();
    case State::ListQ8Tiered: return polar_q8_tiered_kernel_ptr();
    }
    return nullptr;
}

}  // namespace

extern "C" {

// a persistent kernel's grid: per_cu workgroups on each CU, or BCHK_POLAR_GRID workgroups
// (experiments); BCHK_POLAR_DEBUG prints the choice
static int polar_grid(const char *who, const bchk_polar *c, size_t lds, int per_cu, int cus) {
    int grid = per_cu * cus;
    env_int("BCHK_POLAR_GRID", &grid, 1, INT_MAX);
    if (env_flag("BCHK_POLAR_DEBUG"))
        fprintf(stderr, "%s: U=%d L=%d lds=%zu per_cu=%d CUs=%d grid=%d\n", who, c->U, c->L, lds, per_cu, cus, grid);
    return grid;
}

int bchk_polar_create(const char *spec, int list_size, int device, bchk_polar **out) {
    return bchk_polar_create_kdir(spec, nullptr, list_size, device, out);
}

// want: List = every path's state in LDS, through the kernel the code needs (split 0); a tiered
// state with split -1 (the library chooses) or 1..n
static int polar_create(const char *spec, const char *kdir, int list_size, int device, int split, State want,
                        bchk_polar **out);

int bchk_polar_create_kdir(const char *spec, const char *kdir, int list_size, int device, bchk_polar **out) {
    return polar_create(spec, kdir, list_size, device, 0, State::List, out);
}

// the checked entry of the tiered states
static int polar_create_tiered(const char *spec, const char *kdir, int list_size, int device, int split, State want,
                               bchk_polar **out) {
    if (split == 0 || split < -1) {
        if (out) *out = nullptr;
        return pfail(BCHK_EINVAL, "split %d out of range (-1, or 1..layers)", split);
    }
    return polar_create(spec, kdir, list_size, device, split, want, out);
}

int bchk_polar_create_tiered_mixed(const char *spec, const char *kdir, int list_size, int device, int split,
                                   bchk_polar **out) {
    return polar_create_tiered(spec, kdir, list_size, device, split, State::MixedTiered, out);
}

int bchk_polar_create_tiered(const char *spec, const char *kdir, int list_size, int device, int split,
                             bchk_polar **out) {
    return polar_create_tiered(spec, kdir, list_size, device, split, State::ListTiered, out);
}

int bchk_polar_create_q8(const char *spec, const char *kdir, int list_size, int device, bchk_polar **out) {
    return polar_create(spec, kdir, list_size, device, 0, State::ListQ8, out);
}

int bchk_polar_create_q8_tiered(const char *spec, const char *kdir, int list_size, int device, int split,
                                bchk_polar **out) {
    return polar_create_tiered(spec, kdir, list_size, device, split, State::ListQ8Tiered, out);
}

// both int8 states: the first layer that is not Arikan is refused by name
static int q8_all_arikan(const bchk_polar *c, const char *spec) {
    for (int j = 0; j < c->n; ++j)
        if (!c->arikan[j]) {
            std::istringstream in(spec);
            std::string name;
            for (int t = 0; t < 6 + j + 1; ++t) in >> name;  // the header's six numbers, then the layers
            return pfail(BCHK_EINVAL, "the int8 decoder is built for all-Arikan codes: layer %d is \"%s\"", j,
                         name.c_str());
        }
    return 0;
}

static int polar_create(const char *spec, const char *kdir, int list_size, int device, int split, State want,
                        bchk_polar **out) {
    if (!out || !spec) return pfail(BCHK_EINVAL, "NULL argument");
    *out = nullptr;
    if (list_size < 1 || list_size > kPolarMaxList)
        return pfail(BCHK_EINVAL, "list size %d unsupported (1..%d)", list_size, kPolarMaxList);
    // the specification is checked first, so malformed codes are reported with or without a GPU
    std::unique_ptr<bchk_polar, void (*)(bchk_polar *)> ctx(new bchk_polar(), bchk_polar_destroy);
    bchk_polar *const c = ctx.get();
    c->L = list_size;
    c->device = device;
    if (int rc = parse_spec(c, spec, kdir)) return rc;
    if (want == State::MixedTiered) {
        if (split > c->n) return pfail(BCHK_EINVAL, "split %d out of range (-1, or 1..%d)", split, c->n);
        if (int rc = mixed_tables(c)) return rc;
        if (c->mp.any_ml)
            return pfail(BCHK_EINVAL, "the tiered mixed state does not take a code with a search layer (a matrix kernel "
                                      "above %d, or BCHK_POLAR_ML): its save slots cover the LDS state", kPolarMaxTrellisKernel);
        c->state = State::MixedTiered;
        if (split < 0) split = auto_split(c, [&](int s) { return mixed_tiered_lds_at(c, s); });
        c->split = split;
        mixed_tiered_layout(c, split, c->tm);
        c->lds = mixed_tiered_lds(c, c->tm).bytes;
    } else if (want == State::ListTiered || want == State::ListQ8Tiered) {
        const bool q8 = want == State::ListQ8Tiered;
        if (q8) {
            if (int rc = q8_all_arikan(c, spec)) return rc;
        } else if (c->mixed) {
            return pfail(BCHK_EINVAL, "tiered state is built for all-Arikan codes (a matrix or named layer)");
        }
        if (split > c->n) return pfail(BCHK_EINVAL, "split %d out of range (-1, or 1..%d)", split, c->n);
        c->state = want;
        if (split < 0) split = auto_split(c, [&](int s) { return (size_t)tiered_layout(c, s, q8).bytes; });
        c->split = split;
        int32_t off[kPolarMaxLayers + 1];
        (void)polar_cw_layout(c->U, off);
        c->cwall = off[c->n] + 1;
        c->cwsplit = split < c->n ? off[split + 1] : c->cwall;
        c->lds = tiered_layout(c, split, q8).bytes;
    } else if (want == State::ListQ8) {
        if (int rc = q8_all_arikan(c, spec)) return rc;
        c->state = State::ListQ8;
        c->lds = polar_q8_layout(c->U, c->L, c->K, polar_cw_layout(c->U, nullptr)).bytes;
    } else if (c->mixed) {
        if (int rc = mixed_tables(c)) return rc;
        c->state = State::Mixed;
        c->lds = mixed_lds(c).bytes;
    } else {
        c->lds = polar_list_layout(c->U, c->L, c->K, polar_cw_layout(c->U, nullptr)).bytes;
    }
    if (c->lds > kPolarLdsMax) {
        if (c->is_tiered())
            return pfail(BCHK_EINVAL, "length %d with list %d at split %d still needs %zu B of LDS (> 160 KiB)", c->U,
                         list_size, c->split, c->lds);
        return pfail(BCHK_EINVAL, "length %d with list %d needs %zu B of LDS (> 160 KiB)", c->U, list_size, c->lds);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return pfail(BCHK_ENODEV, "no HIP device visible (the SC-list decoder has no CPU fallback)");
    if (device < 0 || device >= ndev) return pfail(BCHK_EINVAL, "device %d out of range", device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return pfail(BCHK_ENODEV, "device %d is not gfx950; libbchk is built for gfx950 only", device);
    if (hipSetDevice(device) != hipSuccess) return pfail(BCHK_EHIP, "hipSetDevice(%d) failed", device);
    // device tables, one blob
    auto al = [](size_t v) { return (v + 15) & ~size_t(15); };
    size_t o = 0;
    c->off_symmap = o; o = al(o + 2 * (size_t)c->U);
    c->off_phase = o; o = al(o + 2 * (size_t)c->U);
    c->off_cwpos = o; o = al(o + 2 * (size_t)c->N);
    c->off_dfcorr = o; o = al(o + 8 * (size_t)c->U);
    c->off_krows = o; o = al(o + 8 * c->krows.size());
    c->off_tent = o; o = al(o + 4 * c->tent.size());
    c->off_tbase = o; o = al(o + 4 * c->tbase.size());
    c->off_tlog = o; o = al(o + c->tlog.size());
    c->off_inforank = o; o = al(o + 2 * (size_t)c->U);
    c->off_dynoff = o; o = al(o + 4 * c->dynoff.size());
    c->off_dynterm = o; o = al(o + 2 * c->dynterm.size() + 2);
    std::vector<uint8_t> blob(o, 0);
    memcpy(blob.data() + c->off_symmap, c->symmap.data(), 2 * (size_t)c->U);
    {
        uint16_t *ph = reinterpret_cast<uint16_t *>(blob.data() + c->off_phase);
        for (int i = 0; i < c->U; ++i)
            ph[i] = (uint16_t)((c->frozen[i] ? kPhaseFrozen : 0u) | ((uint16_t)(c->dfbit[i] + 1) << 1) |
                               (c->dfcorr[i] ? kPhaseCorr : 0u));
    }
    memcpy(blob.data() + c->off_cwpos, c->cwpos.data(), 2 * (size_t)c->N);
    memcpy(blob.data() + c->off_dfcorr, c->dfcorr.data(), 8 * (size_t)c->U);
    memcpy(blob.data() + c->off_krows, c->krows.data(), 8 * c->krows.size());
    if (!c->tent.empty()) memcpy(blob.data() + c->off_tent, c->tent.data(), 4 * c->tent.size());
    if (!c->tbase.empty()) memcpy(blob.data() + c->off_tbase, c->tbase.data(), 4 * c->tbase.size());
    if (!c->tlog.empty()) memcpy(blob.data() + c->off_tlog, c->tlog.data(), c->tlog.size());
    memcpy(blob.data() + c->off_inforank, c->inforank.data(), 2 * (size_t)c->U);
    memcpy(blob.data() + c->off_dynoff, c->dynoff.data(), 4 * c->dynoff.size());
    if (!c->dynterm.empty()) memcpy(blob.data() + c->off_dynterm, c->dynterm.data(), 2 * c->dynterm.size());
    if (hipMalloc(&c->d_tab, o) != hipSuccess ||
        hipMemcpy(c->d_tab, blob.data(), o, hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return pfail(BCHK_EHIP, "device setup failed");
    const void *fn = kernel_ptr(c->state);
    if (c->lds > 65536) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, c->lds) != hipSuccess || per_cu <= 0) {
        per_cu = 1;
        (void)hipGetLastError();
    }
    if (c->is_tiered()) per_cu = std::min(per_cu, kTieredWaves);
    c->grid = polar_grid("bchk_polar", c, c->lds, per_cu, prop.multiProcessorCount);
    if (c->is_tiered()) {
        // one workspace per workgroup, allocated once; the grid shrinks to keep them within the
        // bound (BCHK_POLAR_WORKSPACE_MB, default 1024), down to a single workgroup
        const uint64_t per_wg = ws_bytes(c);
        int mb = 1024;
        env_int("BCHK_POLAR_WORKSPACE_MB", &mb, 1, 1 << 20);
        const uint64_t fit = ((uint64_t)mb << 20) / per_wg;
        if ((uint64_t)c->grid > fit) c->grid = (int)std::max<uint64_t>(fit, 1);
        if (env_flag("BCHK_POLAR_DEBUG"))
            fprintf(stderr, "bchk_polar tiered: split=%d workspace=%llu B x grid %d\n", c->split,
                    (unsigned long long)per_wg, c->grid);
        if (int rc = c->ws.ensure((size_t)(per_wg * (uint64_t)c->grid))) return rc;
    }
    // codes with search layers: launches of at most ~50 ms (BCHK_POLAR_BUDGET_MS, 0 = one
    // launch per call), so no launch holds the GPU for seconds
    if (c->state == State::Mixed && c->mp.any_ml) {
        double ms = 50.0;
        env_double("BCHK_POLAR_BUDGET_MS", &ms, 0.0, DBL_MAX);
        c->budget_ticks = (uint64_t)(ms * 1e5);  // s_memrealtime: 100 MHz
    }
    *out = ctx.release();
    return 0;
}

void bchk_polar_destroy(bchk_polar *c) {
    if (!c) return;
    if (c->d_tab) (void)hipFree(c->d_tab);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bchk_polar_last_launches(const bchk_polar *c, uint64_t *launches) {
    if (!c || !launches) return pfail(BCHK_EINVAL, "NULL argument");
    *launches = c->budget_ticks ? c->launches_last : 1;
    return 0;
}

int bchk_polar_scratch_bytes(const bchk_polar *c, uint64_t *bytes, uint64_t *save_stride) {
    if (!c || !bytes) return pfail(BCHK_EINVAL, "NULL argument");
    *bytes = (uint64_t)c->rstate.cap + c->rsave.cap + c->unfinished.cap + c->ws.cap;
    if (save_stride) *save_stride = (c->mixed && c->mp.any_ml) ? mixed_lds(c).save_bytes : 0;
    return 0;
}

int bchk_polar_params(const bchk_polar *c, int *n, int *k, int *unshortened, int *list_size) {
    if (!c) return pfail(BCHK_EINVAL, "NULL argument");
    if (n) *n = c->N;
    if (k) *k = c->K;
    if (unshortened) *unshortened = c->U;
    if (list_size) *list_size = c->L;
    return 0;
}

// the caller's buffers and the context's tables, as every decode launch takes them
static PolarIo polar_io(const bchk_polar *c, const float *d_llr, uint8_t *d_info, uint8_t *d_cw, float *d_metric,
                        int32_t *d_count) {
    PolarIo io{};
    io.llr = d_llr;
    io.info = d_info;
    io.cw = d_cw;
    io.metric = d_metric;
    io.count = d_count;
    io.symmap = reinterpret_cast<const int16_t *>(c->d_tab + c->off_symmap);
    io.phase = reinterpret_cast<const uint16_t *>(c->d_tab + c->off_phase);
    io.cwpos = reinterpret_cast<const int16_t *>(c->d_tab + c->off_cwpos);
    io.dfcorr = reinterpret_cast<const uint64_t *>(c->d_tab + c->off_dfcorr);
    return io;
}
// the parameter block of the all-Arikan kernels (f32, tiered, int8)
static PolarParams polar_list_params(const bchk_polar *c, const PolarIo &io, size_t B) {
    PolarParams p{};
    p.io = io;
    p.B = (uint32_t)B;
    p.pathCw = polar_cw_layout(c->U, p.cwoff);
    p.n = c->n;
    p.U = c->U;
    p.N = c->N;
    p.K = c->K;
    p.L = c->L;
    return p;
}

int bchk_polar_decode_device(bchk_polar *c, const float *d_llr, size_t B, uint8_t *d_info,
                             uint8_t *d_cw, float *d_metric, int32_t *d_count, void *stream) {
    if (!c || (B && (!d_llr || !d_info || !d_metric || !d_count))) return pfail(BCHK_EINVAL, "NULL argument");
    if (c->is_q8())
        return pfail(BCHK_EINVAL, "an int8 context (bchk_polar_create_q8*) decodes through bchk_polar_decode_q8_* only");
    if (B == 0) return 0;
    if (B > 0xFFFFFFFFull) return pfail(BCHK_EINVAL, "batch too large");
    const PolarIo io = polar_io(c, d_llr, d_info, d_cw, d_metric, d_count);
    const int grid = (int)std::min<size_t>((size_t)c->grid, B);  // tiered: <= the workspaces allocated at create
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    auto list_params = [&]() { return polar_list_params(c, io, B); };
    auto mixed_params = [&](PolarMixedParams m) {  // m: the state's layout
        m.io = io;
        m.krows = reinterpret_cast<const uint64_t *>(c->d_tab + c->off_krows);
        m.tent = reinterpret_cast<const uint32_t *>(c->d_tab + c->off_tent);
        m.tbase = reinterpret_cast<const uint32_t *>(c->d_tab + c->off_tbase);
        m.tlog = c->d_tab + c->off_tlog;
        m.B = (uint32_t)B;
        m.U = c->U;
        m.N = c->N;
        m.K = c->K;
        m.L = c->L;
        return m;
    };
    switch (c->state) {
    case State::List:
        PHIP_TRY(launch_polar(list_params(), grid, c->lds, s));
        return 0;
    case State::ListTiered: {
        PolarTieredParams t{};
        t.p = list_params();
        t.ws = (uint8_t *)c->ws.p;
        t.split = c->split;
        t.cwsplit = c->cwsplit;
        t.cwall = c->cwall;
        PHIP_TRY(launch_polar_tiered(t, grid, c->lds, s));
        return 0;
    }
    case State::MixedTiered: {
        PolarMixedTieredParams t = c->tm;
        t.m = mixed_params(c->tm.m);
        t.ws = (uint8_t *)c->ws.p;
        PHIP_TRY(launch_polar_mixed_tiered(t, grid, c->lds, s));
        return 0;
    }
    case State::Mixed:
    case State::ListQ8:  // (refused above)
    case State::ListQ8Tiered:
        break;
    }
    PolarMixedParams m = mixed_params(c->mp);
    if (!(m.any_ml && c->budget_ticks)) {
        PHIP_TRY(launch_polar_mixed(m, grid, c->lds, s));
        return 0;
    }
    // Codes with search layers: one codeword's list decode can run for seconds (every
    // phase's search items in one wave), so the call is a series of launches of at most
    // ~budget each (plus one search item): a wave suspends its codeword between two items
    // past the budget and the next launch resumes it (same results, bit for bit: the
    // state saved is the whole list state). The call returns when every codeword is done.
    // A workgroup has at most one suspended codeword (PolarMixedParams), and the grid is
    // the same for every launch of the call: one save slot per workgroup.
    const uint32_t stride = mixed_lds(c).save_bytes;
    int rc;
    if ((rc = c->rstate.ensure(B * 4)) || (rc = c->rsave.ensure((size_t)grid * stride)) ||
        (rc = c->unfinished.ensure(8)))
        return rc;
    PHIP_TRY(hipMemsetAsync(c->rstate.p, 0, B * 4, s));
    m.rstate = (uint32_t *)c->rstate.p;
    m.rsave = (uint8_t *)c->rsave.p;
    m.rstride = stride;
    m.unfinished = (uint32_t *)c->unfinished.p;  // two words: unfinished, progress
    m.progress = m.unfinished + 1;
    m.budget = c->budget_ticks;
    m.no_mid = env_flag("BCHK_POLAR_NO_MID") ? 1 : 0;  // per call: tests toggle it on a live context
    for (uint64_t launch = 0;; ++launch) {
        PHIP_TRY(hipMemsetAsync(c->unfinished.p, 0, 8, s));
        PHIP_TRY(launch_polar_mixed(m, grid, c->lds, s));
        uint32_t left[2] = {0, 0};
        PHIP_TRY(hipMemcpyAsync(left, c->unfinished.p, 8, hipMemcpyDeviceToHost, s));
        PHIP_TRY(hipStreamSynchronize(s));
        c->launches_last = launch + 1;
        if (left[0] == 0) break;
        // every launch that leaves work does some (the kernel starts or resumes a wave's
        // first unfinished codeword whatever the clock says): no progress is a kernel fault,
        // reported instead of launching for ever
        if (left[1] == 0)
            return pfail(BCHK_EHIP, "budgeted SC-list decode made no progress in launch %llu (%u codewords left)",
                         (unsigned long long)(launch + 1), left[0]);
    }
    return 0;
}

int bchk_polar_state_info(const bchk_polar *c, int *split, uint64_t *lds_bytes, uint64_t *workspace_bytes, int *grid) {
    if (!c) return pfail(BCHK_EINVAL, "NULL argument");
    if (split) *split = c->is_tiered() ? c->split : 0;
    if (lds_bytes) *lds_bytes = c->lds;
    if (workspace_bytes) *workspace_bytes = ws_bytes(c);
    if (grid) *grid = c->grid;
    return 0;
}

// The int8 decoders (polar_sclist_q8.hip, polar_sclist_q8_tiered.hip): d_llr [B][N] int8, the outputs as
// bchk_polar_decode_device.
int bchk_polar_decode_q8_device(bchk_polar *c, const int8_t *d_llr, size_t B, uint8_t *d_info, uint8_t *d_cw,
                                float *d_metric, int32_t *d_count, void *stream) {
    if (!c || (B && (!d_llr || !d_info || !d_metric || !d_count))) return pfail(BCHK_EINVAL, "NULL argument");
    if (!c->is_q8())
        return pfail(BCHK_EINVAL, "bchk_polar_decode_q8_* take a context of bchk_polar_create_q8* (this one decodes f32 LLRs)");
    if (B == 0) return 0;
    if (B > 0xFFFFFFFFull) return pfail(BCHK_EINVAL, "batch too large");
    const PolarParams lp = polar_list_params(c, polar_io(c, nullptr, d_info, d_cw, d_metric, d_count), B);
    const int grid = (int)std::min<size_t>((size_t)c->grid, B);  // tiered: <= the workspaces allocated at create
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (c->state == State::ListQ8Tiered) {
        PolarQ8TieredParams q{};
        q.t.p = lp;
        q.t.ws = (uint8_t *)c->ws.p;
        q.t.split = c->split;
        q.t.cwsplit = c->cwsplit;
        q.t.cwall = c->cwall;
        q.llr8 = d_llr;
        PHIP_TRY(launch_polar_q8_tiered(q, grid, c->lds, s));
        return 0;
    }
    PolarQ8Params q{};
    q.p = lp;
    q.llr8 = d_llr;
    PHIP_TRY(launch_polar_q8(q, grid, c->lds, s));
    return 0;
}

// both host decodes: rows of `elem` bytes per LLR (4: f32, 1: int8) through the context's buffers
static int polar_decode_host(bchk_polar *c, const void *llr, size_t elem, size_t B, uint8_t *info, uint8_t *cw,
                             float *metric, int32_t *count) {
    if (!c || (B && (!llr || !info || !metric || !count))) return pfail(BCHK_EINVAL, "NULL argument");
    if ((elem == 1) != c->is_q8())  // before any copy; the device entries name the reason
        return elem == 1 ? bchk_polar_decode_q8_device(c, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr)
                         : bchk_polar_decode_device(c, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (B == 0) return 0;
    const size_t L = (size_t)c->L;
    int rc;
    if ((rc = c->llr.ensure(B * c->N * elem)) || (rc = c->info.ensure(B * L * std::max(c->K, 1))) ||
        (rc = c->metric.ensure(B * L * sizeof(float))) || (rc = c->count.ensure(B * sizeof(int32_t))) ||
        (cw && (rc = c->cw.ensure(B * L * c->N))))
        return rc;
    PHIP_TRY(hipMemcpyAsync(c->llr.p, llr, B * c->N * elem, hipMemcpyHostToDevice, c->stream));
    // list rows past each count keep the caller's contents, as the reference leaves them
    PHIP_TRY(hipMemcpyAsync(c->info.p, info, B * L * c->K, hipMemcpyHostToDevice, c->stream));
    PHIP_TRY(hipMemcpyAsync(c->metric.p, metric, B * L * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (cw) PHIP_TRY(hipMemcpyAsync(c->cw.p, cw, B * L * c->N, hipMemcpyHostToDevice, c->stream));
    uint8_t *const d_cw = cw ? (uint8_t *)c->cw.p : nullptr;
    if ((rc = elem == 1 ? bchk_polar_decode_q8_device(c, (const int8_t *)c->llr.p, B, (uint8_t *)c->info.p, d_cw,
                                                      (float *)c->metric.p, (int32_t *)c->count.p, c->stream)
                        : bchk_polar_decode_device(c, (const float *)c->llr.p, B, (uint8_t *)c->info.p, d_cw,
                                                   (float *)c->metric.p, (int32_t *)c->count.p, c->stream)))
        return rc;
    PHIP_TRY(hipMemcpyAsync(info, c->info.p, B * L * c->K, hipMemcpyDeviceToHost, c->stream));
    PHIP_TRY(hipMemcpyAsync(metric, c->metric.p, B * L * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PHIP_TRY(hipMemcpyAsync(count, c->count.p, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (cw) PHIP_TRY(hipMemcpyAsync(cw, c->cw.p, B * L * c->N, hipMemcpyDeviceToHost, c->stream));
    PHIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int bchk_polar_decode_host(bchk_polar *c, const float *llr, size_t B, uint8_t *info, uint8_t *cw,
                           float *metric, int32_t *count) {
    return polar_decode_host(c, llr, sizeof(float), B, info, cw, metric, count);
}

int bchk_polar_decode_q8_host(bchk_polar *c, const int8_t *llr, size_t B, uint8_t *info, uint8_t *cw,
                              float *metric, int32_t *count) {
    return polar_decode_host(c, llr, 1, B, info, cw, metric, count);
}

// q = clamp(rint(llr scale), -qmax, qmax), ties to even, NaN -> 0 (polar_sclist_q8.hip)
int bchk_polar_quantize_device(bchk_polar *c, const float *d_llr, size_t count, float scale, int qmax, int8_t *d_q,
                               void *stream) {
    if (qmax < 1 || qmax > kQ8Max) return pfail(BCHK_EINVAL, "qmax = %d: the int8 range is 1..%d", qmax, kQ8Max);
    if (!(scale > 0.0f) || std::isinf(scale)) return pfail(BCHK_EINVAL, "scale = %g must be positive and finite", scale);
    if (!c || (count && (!d_llr || !d_q))) return pfail(BCHK_EINVAL, "NULL argument");
    if (count == 0) return 0;
    PHIP_TRY(launch_polar_quantize(d_llr, count, scale, qmax, d_q, stream ? (hipStream_t)stream : c->stream));
    return 0;
}

// CMixedKernelEncoder::Encode (MixedKernelEncoder.cpp:142-177) for Arikan layers, host side:
// frozen symbols from their constraints, the transform, then the transmitted symbols.
int bchk_polar_encode_host(const bchk_polar *c, const uint8_t *info, size_t B, uint8_t *cw) {
    if (!c || (B && (!info || !cw))) return pfail(BCHK_EINVAL, "NULL argument");
    std::vector<uint8_t> u(c->U);
    for (size_t b = 0; b < B; ++b) {
        const uint8_t *in = info + b * c->K;
        int k = 0;
        for (int i = 0; i < c->U; ++i) {
            const int ci = c->decision[i];
            if (ci >= 0) {
                uint8_t v = 0;
                for (int t : c->fc[ci]) {
                    if (t == i) break;
                    v ^= u[t];
                }
                u[i] = v;
            } else {
                u[i] = in[k++] & 1;
            }
        }
        // the transform, innermost layer first (MixedKernelEncoder.cpp:159-170): each block of
        // `next` symbols, viewed as l rows of `stride`, becomes (rows) x K
        std::vector<uint8_t> t(c->U);
        for (int L = c->n - 1, stride = 1; L >= 0; --L) {
            const int l = c->ksize[L], next = stride * l;
            const uint64_t *kr = &c->krows[(size_t)L * kPolarMaxKernel];
            for (int b0 = 0; b0 < c->U; b0 += next)
                for (int i = 0; i < l; ++i)
                    for (int s2 = 0; s2 < stride; ++s2) {
                        uint8_t acc = 0;
                        for (int j = 0; j < l; ++j) acc ^= (uint8_t)(u[b0 + j * stride + s2] & ((kr[j] >> i) & 1ull));
                        t[b0 + i * stride + s2] = acc;
                    }
            u.swap(t);
            stride = next;
        }
        for (int i = 0; i < c->N; ++i) cw[b * c->N + i] = u[c->cwpos[i]];
    }
    return 0;
}

}  // extern "C"

namespace {

PolarEncTables enc_tables(const bchk_polar *c) {
    PolarEncTables t{};
    t.inforank = reinterpret_cast<const int16_t *>(c->d_tab + c->off_inforank);
    t.cwpos = reinterpret_cast<const int16_t *>(c->d_tab + c->off_cwpos);
    t.krows = reinterpret_cast<const uint64_t *>(c->d_tab + c->off_krows);
    t.dynoff = reinterpret_cast<const uint32_t *>(c->d_tab + c->off_dynoff);
    t.dynterm = reinterpret_cast<const uint16_t *>(c->d_tab + c->off_dynterm);
    t.ndyn = (int32_t)c->dynoff.size() - 1;
    t.nl = c->n;
    t.U = c->U;
    t.N = c->N;
    t.K = c->K;
    for (int j = 0; j < c->n; ++j) t.ksize[j] = c->ksize[j];
    return t;
}

// the first `need` set bits 0 of flags[0, nb): the words up to and including the one that
// carries the need-th block error (nb when there are fewer)
size_t cut_at_error(const std::vector<uint8_t> &flags, size_t nb, uint64_t need) {
    for (size_t w = 0; w < nb; ++w)
        if ((flags[w] & 1u) && --need == 0) return w + 1;
    return nb;
}

static_assert(BCHK_CHANNEL_AWGN == kPolarChanAwgn && BCHK_CHANNEL_RAYLEIGH == kPolarChanRayleigh &&
                  BCHK_CHANNEL_BSC == kPolarChanBsc, "the kernel's channel ids are the ABI's");
static_assert(kPolarChanFading + BCHK_FADING_BLOCK == kPolarChanBlock &&
                  kPolarChanFading + BCHK_FADING_CORRELATED == kPolarChanCorrelated &&
                  kPolarChanFading + BCHK_FADING_RICIAN == kPolarChanRician,
              "the kernel's fading models follow its channels in the ABI's order");

}  // namespace

namespace bchk {

// (channel, param) of the bchk_polar_*_channel* entry points (polar_design.cpp too), checked
// before anything else of a call.
int polar_check_channel(int channel, double param) {
    if (channel != BCHK_CHANNEL_AWGN && channel != BCHK_CHANNEL_RAYLEIGH && channel != BCHK_CHANNEL_BSC)
        return pfail(BCHK_EINVAL, "channel %d unknown (BCHK_CHANNEL_AWGN, _RAYLEIGH or _BSC)", channel);
    if (channel == BCHK_CHANNEL_BSC && !(param > 0.0 && param <= 0.5))  // NaN fails both
        return pfail(BCHK_EINVAL, "p = %g: the BSC's crossover probability lies in (0, 0.5]", param);
    return 0;
}

// (kind, param) of the bchk_polar_*_fading* entry points, checked before anything else of a call.
int polar_check_fading(int kind, double param) {
    if (kind != BCHK_FADING_BLOCK && kind != BCHK_FADING_CORRELATED && kind != BCHK_FADING_RICIAN)
        return pfail(BCHK_EINVAL, "kind %d unknown (BCHK_FADING_BLOCK, _CORRELATED or _RICIAN)", kind);
    if (kind == BCHK_FADING_BLOCK && !(param >= 1.0 && param == floor(param) && std::isfinite(param)))  // NaN fails
        return pfail(BCHK_EINVAL, "block size %g: an integer of at least 1", param);
    if (kind == BCHK_FADING_CORRELATED && !(param >= 0.0 && param < 1.0))
        return pfail(BCHK_EINVAL, "rho = %g: the correlation coefficient lies in [0, 1)", param);
    if (kind == BCHK_FADING_RICIAN && !(param >= 0.0 && std::isfinite(param)))
        return pfail(BCHK_EINVAL, "K-factor %g: finite and not negative", param);
    return 0;
}

}  // namespace bchk

// Words [word0, word0 + B) of the stream `seed` over the kernel's channel `chan` (kPolarChan*,
// checked by the caller): param = Eb/N0 in dB, on the BSC the crossover probability; fpar = the
// parameter of a fading model.
static int polar_generate(bchk_polar *c, int chan, double param, double fpar, size_t B, uint64_t seed, uint64_t word0,
                          uint8_t *d_info, uint8_t *d_cw, float *d_llr, double *d_h, double *d_y, void *stream) {
    if (d_h && chan != kPolarChanRayleigh && chan < kPolarChanFading)
        return pfail(BCHK_EINVAL, "d_h must be NULL: channel %d has no fading factor", chan);
    if (!c || (B && !d_llr)) return pfail(BCHK_EINVAL, "NULL argument");
    if (B > 0xFFFFFFFFull) return pfail(BCHK_EINVAL, "batch too large");
    if (B == 0) return 0;
    if (c->K <= 0) return pfail(BCHK_EINVAL, "a code of dimension 0 has no Eb/N0");
    PolarGenParams p{};
    p.t = enc_tables(c);
    p.info = d_info;
    p.cw = d_cw;
    p.llr = d_llr;
    p.fade = d_h;
    p.y = d_y;
    p.word0 = word0;
    p.B = (uint32_t)B;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);
    p.gen = 1;
    p.channel = chan;
    p.fblock = 1;
    if (chan == kPolarChanBsc) {
        p.cross = param;
        p.sigma = p.var = 1.0;
    } else {
        p.sigma = sqrt(0.5 * pow(10, -param / 10) * c->N / c->K);
        p.var = p.sigma * p.sigma;  // CModem::SetNoiseVariance (Simulator.cpp:109)
    }
    if (chan == kPolarChanBlock) {  // a block of N or more is the whole word
        p.fblock = fpar < (double)c->N ? (int32_t)fpar : c->N;
    } else if (chan == kPolarChanCorrelated) {
        p.f0 = fpar;
        p.f1 = sqrt(1.0 - fpar * fpar);
    } else if (chan == kPolarChanRician) {  // Omega = 2 s^2 + v^2 = 1, K = v^2 / (2 s^2)
        p.f0 = sqrt(fpar / (fpar + 1.0));
        p.f1 = sqrt(1.0 / (2.0 * (fpar + 1.0)));
    }
    PHIP_TRY(launch_polar_gen(p, stream ? (hipStream_t)stream : c->stream));
    return 0;
}

extern "C" {

// CMixedKernelEncoder::Encode (MixedKernelEncoder.cpp:142-177) on the device
// (polar_channel.hip), bit for bit bchk_polar_encode_host.
int bchk_polar_encode_device(bchk_polar *c, const uint8_t *d_info, size_t B, uint8_t *d_cw, void *stream) {
    if (!c || (B && ((c->K && !d_info) || !d_cw))) return pfail(BCHK_EINVAL, "NULL argument");
    if (B > 0xFFFFFFFFull) return pfail(BCHK_EINVAL, "batch too large");
    if (B == 0) return 0;
    PolarGenParams p{};
    p.t = enc_tables(c);
    p.info_in = d_info;
    p.cw = d_cw;
    p.B = (uint32_t)B;
    PHIP_TRY(launch_polar_gen(p, stream ? (hipStream_t)stream : c->stream));
    return 0;
}

// Words [word0, word0 + B) of the counter-based stream `seed` over `channel`. AWGN and Rayleigh:
// param = Eb/N0 in dB, the noise deviation of CSimulator::SetEbN0 (Simulator.cpp:108, N the
// transmitted length). BSC: param = the crossover probability, noise variance 1 (:114).
int bchk_polar_generate_channel_device(bchk_polar *c, int channel, double param, size_t B, uint64_t seed,
                                       uint64_t word0, uint8_t *d_info, uint8_t *d_cw, float *d_llr, double *d_h,
                                       double *d_y, void *stream) {
    if (int rc = polar_check_channel(channel, param)) return rc;
    return polar_generate(c, channel, param, 0.0, B, seed, word0, d_info, d_cw, d_llr, d_h, d_y, stream);
}

// The same stream over a fading model with a parameter (polar_device.h; include/bchk.h):
// snr_db = the average Eb/N0, every model having E[h^2] = 1.
int bchk_polar_generate_fading_device(bchk_polar *c, int kind, double param, double snr_db, size_t B, uint64_t seed,
                                      uint64_t word0, uint8_t *d_info, uint8_t *d_cw, float *d_llr, double *d_h,
                                      double *d_y, void *stream) {
    if (int rc = polar_check_fading(kind, param)) return rc;
    return polar_generate(c, kPolarChanFading + kind, snr_db, param, B, seed, word0, d_info, d_cw, d_llr, d_h, d_y,
                          stream);
}

int bchk_polar_generate_device(bchk_polar *c, double snr_db, size_t B, uint64_t seed, uint64_t word0,
                               uint8_t *d_info, uint8_t *d_cw, float *d_llr, void *stream) {
    return bchk_polar_generate_channel_device(c, BCHK_CHANNEL_AWGN, snr_db, B, seed, word0, d_info, d_cw, d_llr,
                                              nullptr, nullptr, stream);
}

int bchk_polar_count_device(bchk_polar *c, const uint8_t *d_info_tx, const uint8_t *d_cw_tx, const float *d_llr,
                            const uint8_t *d_info, const uint8_t *d_cw, const int32_t *d_count, size_t B,
                            uint64_t *d_out8, uint8_t *d_flags, void *stream) {
    if (!c || (B && ((c->K && (!d_info_tx || !d_info)) || !d_cw_tx || !d_llr || !d_cw || !d_count || !d_out8)))
        return pfail(BCHK_EINVAL, "NULL argument");
    if (B > 0xFFFFFFFFull) return pfail(BCHK_EINVAL, "batch too large");
    if (B == 0) return 0;
    PolarCountParams p{};
    p.info_tx = d_info_tx;
    p.cw_tx = d_cw_tx;
    p.llr = d_llr;
    p.info = d_info;
    p.cw = d_cw;
    p.count = d_count;
    p.out8 = reinterpret_cast<unsigned long long *>(d_out8);
    p.flags = d_flags;
    p.B = (uint32_t)B;
    p.N = c->N;
    p.K = c->K;
    p.L = c->L;
    PHIP_TRY(launch_polar_count(p, stream ? (hipStream_t)stream : c->stream));
    return 0;
}

// The BPSK simulation loop (CSimulator::Iterate over a range of Eb/N0 or, on the BSC, of
// crossover probabilities) end to end on the device: per point, batches are generated, decoded
// and counted until max_words words or max_errors block errors. The batch that reaches
// max_errors is cut in word order from its per-word flags and its prefix counted again (the
// decoded lists are still in the buffers), and the next point starts at the word after the cut:
// the records depend on the arguments only, not on `batch`.
// q8: each batch's LLRs are quantised (scale, qmax) and decoded by the int8 kernel; the counters
// still read the channel's f32 LLRs.
static int polar_sweep(bchk_polar *c, int channel, double fpar, double snr_from, double snr_step, int points,
                       uint64_t max_words, uint64_t max_errors, uint64_t seed, size_t batch, bchk_polar_point *out,
                       double *seconds, uint64_t *words_decoded, bool q8, float scale, int qmax) {
    // every point's parameter, before any work (only the BSC's has a range); channel = kPolarChan*, a
    // fading model and its fpar checked by the caller
    for (int pt = 0; pt < (channel == BCHK_CHANNEL_BSC && points > 0 ? points : 1) && channel < kPolarChanFading; ++pt)
        if (int rc = polar_check_channel(channel, snr_from + pt * snr_step)) return rc;
    if (!c || !out) return pfail(BCHK_EINVAL, "NULL argument");
    if (q8 != c->is_q8())
        return pfail(BCHK_EINVAL, q8 ? "bchk_polar_sweep_q8_device takes a context of bchk_polar_create_q8*"
                                     : "an int8 context (bchk_polar_create_q8*) sweeps through bchk_polar_sweep_q8_device");
    if (q8)  // scale and qmax, checked as every batch would
        if (int rc = bchk_polar_quantize_device(c, nullptr, 0, scale, qmax, nullptr, nullptr)) return rc;
    if (points <= 0 || max_words == 0 || max_errors == 0)
        return pfail(BCHK_EINVAL, "points, max_words and max_errors must be positive");
    if (c->K <= 0) return pfail(BCHK_EINVAL, "a code of dimension 0 has no Eb/N0");
    const size_t N = (size_t)c->N, K = (size_t)std::max(c->K, 1), L = (size_t)c->L;
    const size_t per_word = 4 * N + L * (K + N) + 4 * L + 4 + K + N + 1;
    size_t Bm = batch;
    if (!Bm) {  // a few waves of the decoder's persistent grid, within 1 GiB of buffers
        Bm = std::max<size_t>(4096, 16 * (size_t)c->grid);
        Bm = std::max<size_t>(1, std::min(Bm, (size_t(1) << 30) / per_word));
    }
    Bm = (size_t)std::min<uint64_t>(std::min<uint64_t>(Bm, max_words), 0xFFFFFFFFull);
    int rc;
    if ((rc = c->llr.ensure(Bm * N * sizeof(float))) || (rc = c->info.ensure(Bm * L * K)) ||
        (rc = c->cw.ensure(Bm * L * N)) || (rc = c->metric.ensure(Bm * L * sizeof(float))) ||
        (rc = c->count.ensure(Bm * sizeof(int32_t))) || (rc = c->txinfo.ensure(Bm * K)) ||
        (rc = c->txcw.ensure(Bm * N)) || (rc = c->flags.ensure(Bm)) || (rc = c->cnt8.ensure(8 * sizeof(uint64_t))) ||
        (q8 && (rc = c->q8.ensure(Bm * N))))
        return rc;
    const hipStream_t s = c->stream;
    uint64_t *d8 = (uint64_t *)c->cnt8.p;
    std::vector<uint8_t> flags;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t word = 0, decoded = 0;
    for (int pt = 0; pt < points; ++pt) {
        bchk_polar_point &r = out[pt];
        r.snr_db = snr_from + pt * snr_step;
        for (uint64_t &v : r.c) v = 0;
        while (r.c[0] < max_words && r.c[1] < max_errors) {
            const size_t nb = (size_t)std::min<uint64_t>(Bm, max_words - r.c[0]);
            uint64_t h[8];
            if ((rc = polar_generate(c, channel, r.snr_db, fpar, nb, seed, word, (uint8_t *)c->txinfo.p,
                                     (uint8_t *)c->txcw.p, (float *)c->llr.p, nullptr, nullptr, s)))
                return rc;
            if (q8) {
                if ((rc = bchk_polar_quantize_device(c, (const float *)c->llr.p, nb * N, scale, qmax, (int8_t *)c->q8.p,
                                                     s)) ||
                    (rc = bchk_polar_decode_q8_device(c, (const int8_t *)c->q8.p, nb, (uint8_t *)c->info.p,
                                                      (uint8_t *)c->cw.p, (float *)c->metric.p, (int32_t *)c->count.p,
                                                      s)))
                    return rc;
            } else if ((rc = bchk_polar_decode_device(c, (const float *)c->llr.p, nb, (uint8_t *)c->info.p,
                                                      (uint8_t *)c->cw.p, (float *)c->metric.p, (int32_t *)c->count.p,
                                                      s))) {
                return rc;
            }
            decoded += nb;
            size_t used = nb;
            for (int pass = 0; pass < 2; ++pass) {  // the whole batch, then its prefix up to the cut
                PHIP_TRY(hipMemsetAsync(d8, 0, 8 * sizeof(uint64_t), s));
                if ((rc = bchk_polar_count_device(c, (const uint8_t *)c->txinfo.p, (const uint8_t *)c->txcw.p,
                                                  (const float *)c->llr.p, (const uint8_t *)c->info.p,
                                                  (const uint8_t *)c->cw.p, (const int32_t *)c->count.p, used, d8,
                                                  pass ? nullptr : (uint8_t *)c->flags.p, s)))
                    return rc;
                PHIP_TRY(hipMemcpyAsync(h, d8, sizeof h, hipMemcpyDeviceToHost, s));
                PHIP_TRY(hipStreamSynchronize(s));
                if (h[0] != used)
                    return pfail(BCHK_EHIP, "counters saw %llu of %zu words", (unsigned long long)h[0], used);
                if (pass || r.c[1] + h[1] < max_errors) break;
                flags.resize(nb);
                PHIP_TRY(hipMemcpyAsync(flags.data(), c->flags.p, nb, hipMemcpyDeviceToHost, s));
                PHIP_TRY(hipStreamSynchronize(s));
                used = cut_at_error(flags, nb, max_errors - r.c[1]);
                if (used == nb) break;
            }
            for (int q = 0; q < 8; ++q) r.c[q] += h[q];
            word += used;
        }
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (words_decoded) *words_decoded = decoded;
    return 0;
}

int bchk_polar_sweep_channel_device(bchk_polar *c, int channel, double snr_from, double snr_step, int points,
                                    uint64_t max_words, uint64_t max_errors, uint64_t seed, size_t batch,
                                    bchk_polar_point *out, double *seconds, uint64_t *words_decoded) {
    if (int rc = polar_check_channel(channel, snr_from)) return rc;  // the id; polar_sweep checks every point
    return polar_sweep(c, channel, 0.0, snr_from, snr_step, points, max_words, max_errors, seed, batch, out, seconds,
                       words_decoded, false, 0.0f, 0);
}

// The same loop over a fading model: the points are average Eb/N0 values in dB.
int bchk_polar_sweep_fading_device(bchk_polar *c, int kind, double param, double snr_from, double snr_step, int points,
                                   uint64_t max_words, uint64_t max_errors, uint64_t seed, size_t batch,
                                   bchk_polar_point *out, double *seconds, uint64_t *words_decoded) {
    if (int rc = polar_check_fading(kind, param)) return rc;
    return polar_sweep(c, kPolarChanFading + kind, param, snr_from, snr_step, points, max_words, max_errors, seed,
                       batch, out, seconds, words_decoded, false, 0.0f, 0);
}

// The same loop through the int8 decoder: generate -> quantize (scale, qmax) -> q8 decode -> count.
int bchk_polar_sweep_q8_device(bchk_polar *c, int channel, double snr_from, double snr_step, int points,
                               uint64_t max_words, uint64_t max_errors, uint64_t seed, size_t batch,
                               bchk_polar_point *out, double *seconds, uint64_t *words_decoded, float scale,
                               int qmax) {
    if (int rc = polar_check_channel(channel, snr_from)) return rc;  // the id; polar_sweep checks every point
    return polar_sweep(c, channel, 0.0, snr_from, snr_step, points, max_words, max_errors, seed, batch, out, seconds,
                       words_decoded, true, scale, qmax);
}

int bchk_polar_sweep_q8_fading_device(bchk_polar *c, int kind, double param, double snr_from, double snr_step,
                                      int points, uint64_t max_words, uint64_t max_errors, uint64_t seed, size_t batch,
                                      bchk_polar_point *out, double *seconds, uint64_t *words_decoded, float scale,
                                      int qmax) {
    if (int rc = polar_check_fading(kind, param)) return rc;
    return polar_sweep(c, kPolarChanFading + kind, param, snr_from, snr_step, points, max_words, max_errors, seed,
                       batch, out, seconds, words_decoded, true, scale, qmax);
}

int bchk_polar_sweep_device(bchk_polar *c, double snr_from, double snr_step, int points, uint64_t max_words,
                            uint64_t max_errors, uint64_t seed, size_t batch, bchk_polar_point *out,
                            double *seconds, uint64_t *words_decoded) {
    return bchk_polar_sweep_channel_device(c, BCHK_CHANNEL_AWGN, snr_from, snr_step, points, max_words, max_errors,
                                           seed, batch, out, seconds, words_decoded);
}

// The genie kernel's layout, LDS size and persistent grid (once per context).
static int genie_setup(bchk_polar *c) {
    if (c->genie_grid) return 0;
    PolarMixedParams m{};
    if (c->mixed)
        m = c->mp;
    else
        mixed_layout(c, m);  // an all-Arikan code in the mixed layout: the same f/g arithmetic
    PolarGenieParams &g = c->gp;
    g.ssize = m.ssize;
    g.csize = m.csize;
    g.osize = m.osize;
    g.tstates = m.tstates;
    for (int j = 0; j <= c->n; ++j) {
        g.outer[j] = m.outer[j];
        g.soff[j] = m.soff[j];
        g.coff[j] = m.coff[j];
    }
    for (int j = 0; j < c->n; ++j) {
        g.ooff[j] = m.ooff[j];
        g.arikan[j] = m.arikan[j];
        g.trellis[j] = m.trellis[j];
        g.named[j] = m.named[j];
        g.foff[j] = m.foff[j];
    }
    const size_t lds = polar_genie_layout(c->U, c->K, g.ssize, g.csize, g.osize, c->n, g.tstates).bytes;
    if (lds > 160 * 1024)
        return pfail(BCHK_EINVAL, "genie-aided SC of length %d needs %zu B of LDS (> 160 KiB)", c->U, lds);
    const void *fn = polar_genie_kernel_ptr();
    if (lds > 65536) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, lds) != hipSuccess || per_cu <= 0) {
        per_cu = 1;
        (void)hipGetLastError();
    }
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0) {
        cus = 1;
        (void)hipGetLastError();
    }
    c->genie_lds = lds;
    c->genie_grid = polar_grid("bchk_polar genie", c, lds, per_cu, cus);
    return 0;
}

// Genie-aided SC of one batch (polar_genie.hip): the decision LLR of every symbol with the
// true earlier symbols fed back, and the per-symbol counters added into d_err / d_soft.
int bchk_polar_genie_device(bchk_polar *c, const uint8_t *d_info_tx, const float *d_llr, size_t B, uint64_t *d_err,
                            int64_t *d_soft, float *d_dec_llr, uint8_t *d_u, void *stream) {
    if (!c || (B && ((c->K && !d_info_tx) || !d_llr || !d_err || !d_soft))) return pfail(BCHK_EINVAL, "NULL argument");
    if (c->mixed && c->mp.any_ml)
        return pfail(BCHK_EINVAL, "genie-aided SC does not take a code with a search layer (a matrix kernel above %d, "
                                  "or BCHK_POLAR_ML)", kPolarMaxTrellisKernel);
    if (B > 0xFFFFFFFFull) return pfail(BCHK_EINVAL, "batch too large");
    if (B == 0) return 0;
    int rc;
    if ((rc = genie_setup(c))) return rc;
    // rows the caller does not want go to scratch the context owns (grown on demand)
    if (!d_dec_llr) {
        if ((rc = c->gdec.ensure(B * (size_t)c->U * sizeof(float)))) return rc;
        d_dec_llr = (float *)c->gdec.p;
    }
    if (!d_u) {
        if ((rc = c->gu.ensure(B * (size_t)c->U))) return rc;
        d_u = (uint8_t *)c->gu.p;
    }
    PolarGenieParams p = c->gp;
    p.t = enc_tables(c);
    p.info_tx = d_info_tx;
    p.llr = d_llr;
    p.dec_llr = d_dec_llr;
    p.u = d_u;
    p.symmap = reinterpret_cast<const int16_t *>(c->d_tab + c->off_symmap);
    p.tent = reinterpret_cast<const uint32_t *>(c->d_tab + c->off_tent);
    p.tbase = reinterpret_cast<const uint32_t *>(c->d_tab + c->off_tbase);
    p.tlog = c->d_tab + c->off_tlog;
    p.B = (uint32_t)B;
    const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PHIP_TRY(launch_polar_genie(p, (int)std::min<size_t>((size_t)c->genie_grid, B), c->genie_lds, s));
    PHIP_TRY(launch_polar_genie_sum(d_dec_llr, d_u, (uint32_t)B, c->U, d_err, d_soft, s));
    return 0;
}

// Words [word0, word0 + words) of the stream `seed` over `channel` (kPolarChan*, checked by the
// caller) at `param` (and fpar, polar_generate) through the genie kernel, in batches; the sums are
// integers, so the result does not depend on `batch`.
static int polar_genie_run(bchk_polar *c, int channel, double param, double fpar, uint64_t words, uint64_t seed,
                           uint64_t word0, size_t batch, uint64_t *err, int64_t *soft, double *seconds) {
    if (!c || !err || !soft) return pfail(BCHK_EINVAL, "NULL argument");
    if (words == 0 || words > (1ull << 31))
        return pfail(BCHK_EINVAL, "words must be 1..2^31 (the soft sums stay inside 64 bits)");
    if (c->mixed && c->mp.any_ml)
        return pfail(BCHK_EINVAL, "genie-aided SC does not take a code with a search layer (a matrix kernel above %d, "
                                  "or BCHK_POLAR_ML)", kPolarMaxTrellisKernel);
    if (c->K <= 0) return pfail(BCHK_EINVAL, "a code of dimension 0 has no Eb/N0");
    int rc;
    if ((rc = genie_setup(c))) return rc;
    const size_t N = (size_t)c->N, K = (size_t)c->K, U = (size_t)c->U;
    size_t Bm = batch;
    if (!Bm) {  // a few rounds of the persistent grid, within 256 MiB of buffers
        Bm = std::max<size_t>(4096, 16 * (size_t)c->genie_grid);
        Bm = std::max<size_t>(1, std::min(Bm, (size_t(1) << 28) / (4 * N + K + 5 * U)));
    }
    Bm = (size_t)std::min<uint64_t>(Bm, words);
    if ((rc = c->llr.ensure(Bm * N * sizeof(float))) || (rc = c->txinfo.ensure(Bm * K)) ||
        (rc = c->gdec.ensure(Bm * U * sizeof(float))) || (rc = c->gu.ensure(Bm * U)) || (rc = c->gsum.ensure(16 * U)))
        return rc;
    const hipStream_t s = c->stream;
    uint64_t *d_err = (uint64_t *)c->gsum.p;
    int64_t *d_soft = (int64_t *)(d_err + U);
    const auto t0 = std::chrono::steady_clock::now();
    PHIP_TRY(hipMemsetAsync(c->gsum.p, 0, 16 * U, s));
    for (uint64_t done = 0; done < words;) {
        const size_t nb = (size_t)std::min<uint64_t>(Bm, words - done);
        if ((rc = polar_generate(c, channel, param, fpar, nb, seed, word0 + done, (uint8_t *)c->txinfo.p, nullptr,
                                 (float *)c->llr.p, nullptr, nullptr, s)) ||
            (rc = bchk_polar_genie_device(c, (const uint8_t *)c->txinfo.p, (const float *)c->llr.p, nb, d_err, d_soft,
                                          nullptr, nullptr, s)))
            return rc;
        done += nb;
    }
    std::vector<uint64_t> h(2 * U);
    PHIP_TRY(hipMemcpyAsync(h.data(), c->gsum.p, 16 * U, hipMemcpyDeviceToHost, s));
    PHIP_TRY(hipStreamSynchronize(s));
    memcpy(err, h.data(), 8 * U);
    memcpy(soft, h.data() + U, 8 * U);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int bchk_polar_genie_run_channel(bchk_polar *c, int channel, double param, uint64_t words, uint64_t seed,
                                 uint64_t word0, size_t batch, uint64_t *err, int64_t *soft, double *seconds) {
    if (int rc = polar_check_channel(channel, param)) return rc;
    return polar_genie_run(c, channel, param, 0.0, words, seed, word0, batch, err, soft, seconds);
}

int bchk_polar_genie_run_fading(bchk_polar *c, int kind, double param, double snr_db, uint64_t words, uint64_t seed,
                                uint64_t word0, size_t batch, uint64_t *err, int64_t *soft, double *seconds) {
    if (int rc = polar_check_fading(kind, param)) return rc;
    return polar_genie_run(c, kPolarChanFading + kind, snr_db, param, words, seed, word0, batch, err, soft, seconds);
}

int bchk_polar_genie_run(bchk_polar *c, double snr_db, uint64_t words, uint64_t seed, uint64_t word0, size_t batch,
                         uint64_t *err, int64_t *soft, double *seconds) {
    return bchk_polar_genie_run_channel(c, BCHK_CHANNEL_AWGN, snr_db, words, seed, word0, batch, err, soft, seconds);
}

int bchk_polar_sync(bchk_polar *c) {
    if (!c) return pfail(BCHK_EINVAL, "NULL argument");
    PHIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

void *bchk_polar_stream(bchk_polar *c) { return c ? (void *)c->stream : nullptr; }

}  // extern "C"
