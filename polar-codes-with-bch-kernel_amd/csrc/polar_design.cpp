// polar_design.cpp -- BEC design of polar codes over mixed kernels, host side (include/bchk.h,
// the bchk_kernel_bec_capacity / bchk_kernel_write_file / bchk_polar_design_bec block): the
// capacity evaluation of a kernel's BEC polarisation table, the kernel-file writer that stores
// that table where the reference reads it, and the layer-by-layer capacity recursion that
// picks the frozen set of a code specification. Also the Monte-Carlo design over a simulated
// channel (bchk_polar_design_genie, _channel, _fading): the frozen set ranked by
// the genie-aided error statistics of bchk_polar_genie_run_channel (polar_host.cpp,
// polar_genie.hip).
//
// Reference: CBECCapacityEvaluator (out/external/CapacityEvaluator.cpp:100-140: the table's
// file layout and GetSubchannelCapacity's Horner rule), CArikanKernel::GetSubchannelCapacity
// (out/external/Kernel.cpp:57-79, ec_BEC), CMatrixBinaryKernel's file reader (Kernel.cpp:93-134:
// size, matrix, then per-channel sections, ec_BEC = 3 in headers/external/Simulator.h:13-17).
// The Horner rule is restated and pinned to the compiled reference evaluator, and the writer to
// the reference's reader, by tests/golden/polar_ref_capacity_*.txt.gz (tests/test_polar_design.py):
// equal bits on every recorded row but C = 0. The design recursion does not use that rule for
// matrix layers (design_row below): it is accurate only for capacities near 1/2. The tables
// themselves come from csrc/kernel_bec.hip.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "bchk.h"

namespace bchk {
void set_last_error(const char *msg);  // bchk_host.cpp
int polar_check_channel(int channel, double param);  // polar_host.cpp
int polar_check_fading(int kind, double param);
}

namespace {

constexpr int kMaxKernel = 64;    // read_kernel's bound (polar_host.cpp)
constexpr int kMaxLayers = 14;    // parse_spec's bounds
constexpr long kMaxLength = 16384;
constexpr unsigned kChannelBec = 3;  // ec_BEC

int dfail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    bchk::set_last_error(buf);
    return code;
}

// GetSubchannelCapacity (CapacityEvaluator.cpp:124-140) on one phase's row u[0..l] (u[w] =
// uncorrectable patterns of weight w): 1 - sum_w u[w] P^w C^(l-w), P = 1 - C, by Horner in
// S = P / C; u[0] is not read (the file stores a 0 there, :107). At C = 0, where S is not
// finite, the polynomial's value 1 - u[l]; at C = 1 the rule itself gives 1.
double capacity_row(const double *u, int l, double C) {
    if (C <= 0.0) return 1.0 - u[l];
    const double P = 1.0 - C, S = P / C;
    double E = 0.0;
    for (int i = l; i > 0; --i) {
        E *= S;
        E += u[i];
    }
    E *= S * std::pow(C, l);
    return 1.0 - E;
}

struct Layer {
    bool arikan = true;
    int l = 2;
    std::vector<double> tab;  // [l][l + 1], matrix layers
    std::vector<double> cor;  // [l][l + 1]: C(l, w) - tab, the correctable patterns, clamped at 0
};

// The same capacity as the sum over the CORRECTABLE patterns, sum_w d[w] P^w C^(l-w) with
// d[w] = C(l, w) - u[w] >= 0: no term is negative, so nothing cancels, and the value keeps its
// relative accuracy down to underflow, where capacity_row's 1 - E is rounding noise once the
// capacity falls below 1e-16 and NaN once S^l overflows. The larger of P and C is factored out,
// so Horner runs in a ratio r <= 1 and the one power taken is of a number >= 1/2: nothing
// overflows, and nothing underflows before the result does. At C = 0 this is d[l] = 1 - u[l],
// at C = 1 d[0] = 1. For l <= 56 the d[w] are exact; the relative error is then at most
// (5 l + 4) 2^-53: r carries 2 roundings and each of the at most l multiplications one more, l
// additions of non-negative terms, the base of the power one rounding taken l times, pow and
// the last product.
double design_row(const double *d, int l, double C) {
    const double P = 1.0 - C;
    double E;
    if (C <= P) {
        const double r = C / P;
        E = d[0];
        for (int w = 1; w <= l; ++w) E = E * r + d[w];
        E *= std::pow(P, l);
    } else {
        const double r = P / C;
        E = d[l];
        for (int w = l - 1; w >= 0; --w) E = E * r + d[w];
        E *= std::pow(C, l);
    }
    return E < 1.0 ? E : 1.0;  // E >= 0: every operand is
}

// C(l, w) - tab per phase; a sampled table's estimate may pass C(l, w) by rounding
void correctable_table(Layer &L) {
    const int l = L.l;
    std::vector<long double> binom(l + 1, 1.0L);
    for (int w = 1; w <= l; ++w) binom[w] = binom[w - 1] * (long double)(l - w + 1) / (long double)w;
    L.cor.resize(L.tab.size());
    for (int i = 0; i < l; ++i)
        for (int w = 0; w <= l; ++w) {
            // the file stores a 0 at w = 0 whatever the table holds there; no phase is lost unerased
            const long double v = binom[w] - (w ? (long double)L.tab[(size_t)i * (l + 1) + w] : 0.0L);
            L.cor[(size_t)i * (l + 1) + w] = v > 0.0L ? (double)v : 0.0;
        }
}

// T_phase(C) of one layer (Kernel.cpp:70-75 for the Arikan kernel)
double layer_capacity(const Layer &L, int phase, double C) {
    if (L.arikan) return phase == 0 ? C * C : 2 * C - C * C;
    return design_row(&L.cor[(size_t)phase * (L.l + 1)], L.l, C);
}

// A matrix kernel file (Kernel.cpp:93-134): the size, the matrix, then channel sections; the
// ec_BEC section is l rows "0 u_1 .. u_l" (CapacityEvaluator.cpp:100-117). *has_tab = a
// complete BEC section was read; anything else after the matrix ends the parse, as a failed
// section does in the reference.
int read_kernel_file(const std::string &name, const char *kdir, int *size, std::vector<uint8_t> &K,
                     std::vector<double> &tab, bool *has_tab) {
    std::string path = name.substr(1);
    if (!path.empty() && path[0] != '/' && kdir && kdir[0]) path = std::string(kdir) + "/" + path;
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return dfail(BCHK_EINVAL, "Error reading kernel file %s", path.c_str());
    int l = 0;
    if (fscanf(f, "%d", &l) != 1 || l < 2 || l > kMaxKernel) {
        fclose(f);
        return dfail(BCHK_EINVAL, "Error reading kernel file %s (size)", path.c_str());
    }
    K.assign((size_t)l * l, 0);
    for (int i = 0; i < l * l; ++i) {
        unsigned v;
        if (fscanf(f, "%u", &v) != 1) {
            fclose(f);
            return dfail(BCHK_EINVAL, "Error parsing kernel file %s", path.c_str());
        }
        K[i] = v ? 1 : 0;
    }
    *size = l;
    *has_tab = false;
    unsigned channel;
    if (fscanf(f, "%u", &channel) == 1 && channel == kChannelBec) {
        tab.assign((size_t)l * (l + 1), 0.0);
        bool ok = true;
        for (int i = 0; i < l && ok; ++i)
            for (int w = 0; w <= l && ok; ++w) ok = fscanf(f, "%lf", &tab[(size_t)i * (l + 1) + w]) == 1 && (w > 0 || tab[(size_t)i * (l + 1)] == 0.0);
        *has_tab = ok;
    }
    fclose(f);
    return BCHK_OK;
}

// the size of a kernel the library names besides "A" (Kernel.cpp:253-274, any case): "G" 3,
// "A5" 5 (TruncatedArikanKernel.cpp), else 0
int named_kernel_size(const std::string &name) {
    std::string low = name;
    for (char &ch : low) ch = (char)tolower((unsigned char)ch);
    return low == "g" ? 3 : low == "a5" ? 5 : 0;
}

bool invertible(const std::vector<uint8_t> &K, int l) {
    std::vector<uint64_t> a(l, 0);
    for (int r = 0; r < l; ++r)
        for (int c = 0; c < l; ++c)
            if (K[(size_t)r * l + c]) a[r] |= 1ull << c;
    for (int col = 0, r0 = 0; col < l; ++col, ++r0) {
        int piv = r0;
        while (piv < l && !((a[piv] >> col) & 1ull)) ++piv;
        if (piv == l) return false;
        std::swap(a[piv], a[r0]);
        for (int r = 0; r < l; ++r)
            if (r != r0 && ((a[r] >> col) & 1ull)) a[r] ^= a[r0];
    }
    return true;
}

// The BEC table of K from the GPU: exact up to 32, sampled estimates unc C(l, w) / tried above.
int device_table(const std::vector<uint8_t> &K, int l, uint64_t samples, uint64_t seed, int device, std::vector<double> &tab) {
    tab.assign((size_t)l * (l + 1), 0.0);
    std::vector<uint64_t> cnt((size_t)l * (l + 1));
    if (l <= 32) {
        if (int rc = bchk_kernel_bec_behaviour(K.data(), l, 0, l, device, cnt.data())) return rc;
        for (size_t i = 0; i < cnt.size(); ++i) tab[i] = (double)cnt[i];
        return BCHK_OK;
    }
    std::vector<uint64_t> tried(l + 1);
    std::vector<uint8_t> exact(l + 1);
    if (int rc = bchk_kernel_bec_sample(K.data(), l, samples, seed, device, cnt.data(), tried.data(), exact.data(), 0, nullptr)) return rc;
    std::vector<long double> binom(l + 1, 1.0L);  // C(l, w)
    for (int w = 1; w <= l; ++w) binom[w] = binom[w - 1] * (long double)(l - w + 1) / (long double)w;
    for (int i = 0; i < l; ++i)
        for (int w = 0; w <= l; ++w)
            tab[(size_t)i * (l + 1) + w] = exact[w] ? (double)cnt[(size_t)i * (l + 1) + w]
                                                    : (double)((long double)cnt[(size_t)i * (l + 1) + w] * binom[w] / (long double)tried[w]);
    return BCHK_OK;
}

}  // namespace

extern "C" {

int bchk_kernel_bec_capacity(const uint64_t *counts, int l, int phase, double C, double *out) {
    if (!counts || !out) return dfail(BCHK_EINVAL, "NULL argument");
    if (l < 2 || l > kMaxKernel || phase < 0 || phase >= l) return dfail(BCHK_EINVAL, "phase %d of a kernel of size %d", phase, l);
    if (!(C >= 0.0 && C <= 1.0)) return dfail(BCHK_EINVAL, "capacity %g outside [0, 1]", C);
    double u[kMaxKernel + 1];
    for (int w = 0; w <= l; ++w) u[w] = (double)counts[(size_t)phase * (l + 1) + w];
    *out = capacity_row(u, l, C);
    return BCHK_OK;
}

int bchk_kernel_write_file(const char *path, const uint8_t *K, int l, const uint64_t *counts) {
    if (!path || !K) return dfail(BCHK_EINVAL, "NULL argument");
    if (l < 2 || l > kMaxKernel) return dfail(BCHK_EINVAL, "kernel size %d unsupported (2..%d)", l, kMaxKernel);
    FILE *f = fopen(path, "w");
    if (!f) return dfail(BCHK_EINVAL, "cannot write %s", path);
    fprintf(f, "%d\n", l);
    for (int r = 0; r < l; ++r)
        for (int c = 0; c < l; ++c) fprintf(f, "%d%c", K[(size_t)r * l + c] ? 1 : 0, c + 1 < l ? ' ' : '\n');
    if (counts) {
        fprintf(f, "%u\n", kChannelBec);
        for (int i = 0; i < l; ++i) {
            fprintf(f, "0");
            for (int w = 1; w <= l; ++w) fprintf(f, " %llu", (unsigned long long)counts[(size_t)i * (l + 1) + w]);
            fprintf(f, "\n");
        }
    }
    if (fclose(f) != 0) return dfail(BCHK_EINVAL, "error writing %s", path);
    return BCHK_OK;
}

int bchk_polar_design_bec(const char *layers, const char *kdir, int K, double capacity, uint64_t samples, uint64_t seed,
                          int device, double *cap, char *spec, size_t spec_len, size_t *needed) {
    if (needed) *needed = 0;
    if (!layers || !needed) return dfail(BCHK_EINVAL, "NULL argument");
    if (!(capacity >= 0.0 && capacity <= 1.0)) return dfail(BCHK_EINVAL, "capacity %g outside [0, 1]", capacity);
    std::istringstream in(layers);
    std::vector<std::string> names;
    for (std::string s; in >> s;) names.push_back(s);
    const int n = (int)names.size();
    if (n < 1 || n > kMaxLayers) return dfail(BCHK_EINVAL, "%d layers unsupported", n);
    std::vector<Layer> L(n);
    std::map<std::string, int> seen;  // a file named twice is read (and measured) once
    long U = 1;
    for (int j = 0; j < n; ++j) {
        const std::string &name = names[j];
        if (name == "A" || name == "a") {
            U *= 2;
        } else if (name[0] == '-' || name[0] == '<') {
            const auto it = seen.find(name.substr(1));
            if (it != seen.end()) {
                L[j] = L[it->second];
            } else {
                std::vector<uint8_t> Km;
                bool has = false;
                L[j].arikan = false;
                if (int rc = read_kernel_file(name, kdir, &L[j].l, Km, L[j].tab, &has)) return rc;
                if (!invertible(Km, L[j].l)) return dfail(BCHK_EINVAL, "Kernel is singular (%s)", name.c_str() + 1);
                if (!has)
                    if (int rc = device_table(Km, L[j].l, samples, seed, device, L[j].tab)) return rc;
                correctable_table(L[j]);
                seen[name.substr(1)] = j;
            }
            U *= L[j].l;
        } else if (named_kernel_size(name)) {
            // the library's BEC table of a named kernel is program text, and the ML polarisation
            // of its matrix is not what its f/g processor achieves (A5): no BEC design here
            return dfail(BCHK_EINVAL, "BEC design does not take the named kernel %s (its decoder is an f/g processor, "
                                      "not ML over the matrix); use bchk_polar_design_genie", name.c_str());
        } else {
            return dfail(BCHK_EINVAL, "Unknown kernel %s", name.c_str());
        }
        if (U > kMaxLength) return dfail(BCHK_EINVAL, "length %ld exceeds %ld", U, kMaxLength);
    }
    if (K < 0 || K > U) return dfail(BCHK_EINVAL, "Code dimension cannot exceed code length");
    // Symbol i = (a_0 .. a_{n-1}), a_0 most significant. Layer 0 is applied last by the encoder
    // with the largest stride (polar_host.cpp bchk_polar_encode_host), so it faces the channel:
    // capacity(i) = T_{n-1,a_{n-1}}( .. T_{1,a_1}(T_{0,a_0}(capacity))).
    std::vector<double> c(1, capacity), nx;
    for (int j = 0; j < n; ++j) {
        nx.resize(c.size() * L[j].l);
        for (size_t i = 0; i < c.size(); ++i)
            for (int a = 0; a < L[j].l; ++a) nx[i * L[j].l + a] = layer_capacity(L[j], a, c[i]);
        c.swap(nx);
    }
    if (cap) std::copy(c.begin(), c.end(), cap);
    // the K largest capacities carry information; ties go to the higher index
    std::vector<int> order(U);
    for (int i = 0; i < U; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return c[a] != c[b] ? c[a] > c[b] : a > b; });
    std::vector<int> frozen(order.begin() + K, order.end());
    std::sort(frozen.begin(), frozen.end());
    std::string text = std::to_string(U) + " " + std::to_string(K) + " 0 " + std::to_string(n) + " 0 0\n";
    for (int j = 0; j < n; ++j) text += names[j] + (j + 1 < n ? " " : "\n");
    for (int f : frozen) text += "1 " + std::to_string(f) + "\n";
    *needed = text.size() + 1;
    if (!spec || spec_len < *needed) return dfail(BCHK_EINVAL, "specification needs %zu bytes, buffer has %zu", *needed, spec ? spec_len : (size_t)0);
    std::memcpy(spec, text.c_str(), *needed);
    return BCHK_OK;
}

// Monte-Carlo design: the symbols ranked by their genie-aided error statistics
// (bchk_polar_genie_run_channel) over `words` words of the stream `seed` over `channel` at
// `param`, decoded as the code with the lowest indices frozen (the rate K / U fixes the noise
// deviation; the statistics do not depend on the frozen set, every earlier symbol being fed
// back true). fading: (channel, fpar) = (kind, param) of a fading model, param its Eb/N0; both
// checked by the caller.
static int design_genie(const char *layers, const char *kdir, int K, bool fading, int channel, double param,
                        double fpar, uint64_t words, uint64_t seed, int device, uint64_t *err, int64_t *soft,
                        char *spec, size_t spec_len, size_t *needed) {
    if (!layers || !needed) return dfail(BCHK_EINVAL, "NULL argument");
    if (words == 0 || words > (1ull << 31)) return dfail(BCHK_EINVAL, "words must be 1..2^31");
    std::istringstream in(layers);
    std::vector<std::string> names;
    for (std::string s; in >> s;) names.push_back(s);
    const int n = (int)names.size();
    if (n < 1 || n > kMaxLayers) return dfail(BCHK_EINVAL, "%d layers unsupported", n);
    long U = 1;
    for (int j = 0; j < n; ++j) {
        const std::string &name = names[j];
        if (name == "A" || name == "a") {
            U *= 2;
        } else if (name[0] == '-' || name[0] == '<') {
            std::vector<uint8_t> Km;
            std::vector<double> tab;
            bool has = false;
            int l = 0;
            if (int rc = read_kernel_file(name, kdir, &l, Km, tab, &has)) return rc;
            if (!invertible(Km, l)) return dfail(BCHK_EINVAL, "Kernel is singular (%s)", name.c_str() + 1);
            U *= l;
        } else if (named_kernel_size(name)) {
            U *= named_kernel_size(name);
        } else {
            return dfail(BCHK_EINVAL, "Unknown kernel %s", name.c_str());
        }
        if (U > kMaxLength) return dfail(BCHK_EINVAL, "length %ld exceeds %ld", U, kMaxLength);
    }
    if (K <= 0 || K > U) return dfail(BCHK_EINVAL, "dimension %d outside 1..%ld", K, U);
    std::string head = std::to_string(U) + " " + std::to_string(K) + " 0 " + std::to_string(n) + " 0 0\n";
    for (int j = 0; j < n; ++j) head += names[j] + (j + 1 < n ? " " : "\n");
    std::string base = head;
    for (long f = 0; f < U - K; ++f) base += "1 " + std::to_string(f) + "\n";
    bchk_polar *pc = nullptr;
    if (int rc = bchk_polar_create_kdir(base.c_str(), kdir, 1, device, &pc)) return rc;
    std::vector<uint64_t> e(U);
    std::vector<int64_t> s(U);
    const int rc = fading ? bchk_polar_genie_run_fading(pc, channel, fpar, param, words, seed, 0, 0, e.data(), s.data(),
                                                        nullptr)
                          : bchk_polar_genie_run_channel(pc, channel, param, words, seed, 0, 0, e.data(), s.data(),
                                                         nullptr);
    bchk_polar_destroy(pc);
    if (rc) return rc;
    // i is better than j: fewer errors, then the larger soft sum, then the higher index
    std::vector<int> order(U);
    for (int i = 0; i < U; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        if (e[a] != e[b]) return e[a] < e[b];
        if (s[a] != s[b]) return s[a] > s[b];
        return a > b;
    });
    std::vector<int> frozen(order.begin() + K, order.end());
    std::sort(frozen.begin(), frozen.end());
    std::string text = head;
    for (int f : frozen) text += "1 " + std::to_string(f) + "\n";
    *needed = text.size() + 1;
    if (!spec || spec_len < *needed) return dfail(BCHK_EINVAL, "specification needs %zu bytes, buffer has %zu", *needed, spec ? spec_len : (size_t)0);
    std::memcpy(spec, text.c_str(), *needed);
    if (err) std::copy(e.begin(), e.end(), err);
    if (soft) std::copy(s.begin(), s.end(), soft);
    return BCHK_OK;
}

int bchk_polar_design_genie_channel(const char *layers, const char *kdir, int K, int channel, double param,
                                    uint64_t words, uint64_t seed, int device, uint64_t *err, int64_t *soft,
                                    char *spec, size_t spec_len, size_t *needed) {
    if (needed) *needed = 0;
    if (int rc = bchk::polar_check_channel(channel, param)) return rc;
    return design_genie(layers, kdir, K, false, channel, param, 0.0, words, seed, device, err, soft, spec, spec_len,
                        needed);
}

int bchk_polar_design_genie_fading(const char *layers, const char *kdir, int K, int kind, double param, double snr_db,
                                   uint64_t words, uint64_t seed, int device, uint64_t *err, int64_t *soft, char *spec,
                                   size_t spec_len, size_t *needed) {
    if (needed) *needed = 0;
    if (int rc = bchk::polar_check_fading(kind, param)) return rc;
    return design_genie(layers, kdir, K, true, kind, snr_db, param, words, seed, device, err, soft, spec, spec_len,
                        needed);
}

int bchk_polar_design_genie(const char *layers, const char *kdir, int K, double snr_db, uint64_t words, uint64_t seed,
                            int device, uint64_t *err, int64_t *soft, char *spec, size_t spec_len, size_t *needed) {
    return bchk_polar_design_genie_channel(layers, kdir, K, BCHK_CHANNEL_AWGN, snr_db, words, seed, device, err, soft,
                                           spec, spec_len, needed);
}

}  // extern "C"
