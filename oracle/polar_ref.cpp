/* polar_ref.cpp -- TEST INFRASTRUCTURE ONLY. Our own driver around the reference's vendored
 * polar library (out/external/*.cpp, headers/external/*.h of the reference tree), linked by
 * oracle/Makefile into oracle/_ref/polar_ref together with twelve of that library's
 * translation units, read in place and compiled with -DOPERATION_COUNTING (the macros of
 * headers/external/misc.h:83-95 only increment counters). It holds no text of the library. oracle/make_golden.py
 * `polar` runs it to write the tests/golden/polar_ref_*.txt.gz fixtures;
 * tests/test_polar_reference.py re-runs it where it is present.
 *
 * Kernel files named "-name.txt" in a specification resolve as the library resolves them:
 * relative to the working directory (Kernel.cpp:93-95, :255-261).
 *
 *   polar_ref decode SPEC L    stdin: one row of N channel LLRs per line, each the hex
 *       bits of an f32. Per row: "D <Decode's return value>", then one line per list
 *       entry, in list order: "<information bits> <codeword bits> <metric, f32 hex bits>".
 *       The metric is read from the decoder's protected m_pSortingBuffer, which after
 *       Decode holds the final (score, path) pairs in list order
 *       (MixedKernelListDecoder.cpp:253-257); a subclass can see it.
 *   polar_ref encode SPEC      stdin: one information word (K bits) per line; per word the
 *       codeword bits of CMixedKernelEncoder::Encode.
 *   polar_ref trellis KERNEL   stdin: per line "<u: size bits> <y: size f32 hex words>".
 *       Calls CTrellisKernelProcessor::GetLLRs (stride 1) at phases 0 .. size-1 in order on
 *       one state variable, with u as the known inputs, and prints the size results as
 *       f32 hex bits: entry p is the LLR of input p given u_0 .. u_{p-1} and y.
 *   polar_ref counts KERNEL    stdin: one row of size channel LLRs per line, f32 hex. Per row
 *       the growth of the library's SumCount and CmpCount (misc.h:76-77) over GetLLRs
 *       (stride 1) at phases 0 .. size-1 in order on one state variable with all-zero known
 *       inputs, as the column search scores a kernel (root bchCoder.cpp:505-515, :641-653):
 *       "<Sum> <Cmp>".
 *   polar_ref capacity KERNEL  stdin: one channel capacity per line, the hex bits of an f64.
 *       The kernel file goes through the library's own reader (CMatrixBinaryKernel(file),
 *       Kernel.cpp:93-134); per line GetSubchannelCapacity(ec_BEC, phase, capacity) of every
 *       phase, as f64 hex bits. The reader only warns when it rejects a BEC section; the
 *       evaluator is then absent, GetSubchannelCapacity throws, and the exit status is 2.
 *
 * Exit status 0, or 2 with the library's message on stderr.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "MixedKernelListDecoder.h"
#include "TrellisKernelProcessor.h"

/* The one symbol the twelve translation units leave undefined: a generator call of the
 * channel simulator. It is on no path a mode takes, so it says its name and aborts; fixture
 * generation never gets there. (CapacityEvaluator.cpp is compiled as it stands; its AWGN half
 * interpolates through oracle/vendored_shim/gsl/gsl_interp.h, at start-up, for the tables of
 * the built-in "G" and "A5" kernels.) */
#define POLAR_REF_STUB(name)                                               \
    do {                                                                   \
        std::fprintf(stderr, "polar_ref: stub reached: %s\n", name);       \
        std::abort();                                                      \
    } while (0)

unsigned long gsl_rng_uniform_int(gsl_rng *, unsigned long) { POLAR_REF_STUB("gsl_rng_uniform_int"); }

namespace {

struct Decoder : CMixedKernelListDecoder {
    Decoder(std::istream &spec, unsigned L) : CMixedKernelListDecoder(spec, L) {}
    float metric(unsigned i) const { return m_pSortingBuffer[i].first; }
};

uint32_t f32_bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

float f32_from_hex(const std::string &s) {
    uint32_t b = (uint32_t)std::strtoul(s.c_str(), nullptr, 16);
    float v;
    std::memcpy(&v, &b, 4);
    return v;
}

void put_bits(const tBit *p, unsigned n) {
    for (unsigned i = 0; i < n; ++i) std::putchar(p[i] ? '1' : '0');
}

bool get_bits(const std::string &s, unsigned n, tBit *out) {
    if (s.size() != n) return false;
    for (unsigned i = 0; i < n; ++i) {
        if (s[i] != '0' && s[i] != '1') return false;
        out[i] = s[i] == '1' ? BIT_1 : BIT_0;
    }
    return true;
}

int usage() {
    std::fprintf(stderr, "usage: polar_ref decode SPEC L | encode SPEC | trellis KERNEL | counts KERNEL | capacity KERNEL  (rows on stdin)\n");
    return 2;
}

int run_decode(const char *specfile, unsigned L) {
    std::ifstream spec(specfile);
    if (!spec) throw Exception("cannot open %s", specfile);
    Decoder dec(spec, L);
    const unsigned N = dec.GetLength(), K = dec.GetDimension();
    std::vector<float> llr(N);
    std::vector<tBit> info((size_t)L * K + 1), cw((size_t)L * N);
    std::string line, w;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        unsigned n = 0;
        while (n < N && (is >> w)) llr[n++] = f32_from_hex(w);
        if (n != N || (is >> w)) throw Exception("a row must hold %d LLRs", N);
        const int ret = dec.Decode(llr.data(), info.data(), cw.data());
        std::printf("D %d\n", ret);
        for (int i = 0; i < ret; ++i) {
            put_bits(info.data() + (size_t)i * K, K);
            std::putchar(' ');
            put_bits(cw.data() + (size_t)i * N, N);
            std::printf(" %08x\n", f32_bits(dec.metric((unsigned)i)));
        }
    }
    return 0;
}

int run_encode(const char *specfile) {
    std::ifstream spec(specfile);
    if (!spec) throw Exception("cannot open %s", specfile);
    CMixedKernelEncoder enc(spec);
    const unsigned N = enc.GetLength(), K = enc.GetDimension();
    std::vector<tBit> info(K + 1), cw(N);
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() && K) continue;
        if (!get_bits(line, K, info.data())) throw Exception("an information word must hold %d bits", K);
        enc.Encode(info.data(), cw.data());
        put_bits(cw.data(), N);
        std::putchar('\n');
    }
    return 0;
}

int run_trellis(const char *kernelfile) {
    CMatrixBinaryKernel kern(kernelfile);
    CTrellisKernelProcessor proc(kern);
    const unsigned l = kern.Size();
    void *state = proc.GetState(1), *temp = proc.GetTemp(1);
    std::vector<tBit> u(l);
    std::vector<float> y(l);
    std::string line, w;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        if (!(is >> w) || !get_bits(w, l, u.data())) throw Exception("known inputs must hold %d bits", l);
        unsigned n = 0;
        while (n < l && (is >> w)) y[n++] = f32_from_hex(w);
        if (n != l || (is >> w)) throw Exception("a row must hold %d LLRs", l);
        for (unsigned p = 0; p < l; ++p) {
            float out = 0;
            proc.GetLLRs(1, p, u.data(), y.data(), &out, state, temp);
            std::printf(p ? " %08x" : "%08x", f32_bits(out));
        }
        std::putchar('\n');
    }
    proc.FreeState(state);
    proc.FreeTemp(temp);
    return 0;
}

int run_counts(const char *kernelfile) {
    CMatrixBinaryKernel kern(kernelfile);
    CTrellisKernelProcessor proc(kern);
    const unsigned l = kern.Size();
    void *state = proc.GetState(1), *temp = proc.GetTemp(1);
    std::vector<tBit> u(l, BIT_0);
    std::vector<float> y(l);
    std::string line, w;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        unsigned n = 0;
        while (n < l && (is >> w)) y[n++] = f32_from_hex(w);
        if (n != l || (is >> w)) throw Exception("a row must hold %d LLRs", l);
        const unsigned long long sum = SumCount, cmp = CmpCount;
        for (unsigned p = 0; p < l; ++p) {
            float out = 0;
            proc.GetLLRs(1, p, u.data(), y.data(), &out, state, temp);
        }
        std::printf("%llu %llu\n", SumCount - sum, CmpCount - cmp);
    }
    proc.FreeState(state);
    proc.FreeTemp(temp);
    return 0;
}

int run_capacity(const char *kernelfile) {
    CMatrixBinaryKernel kern(kernelfile);
    const unsigned l = kern.Size();
    kern.GetSubchannelCapacity(ec_BEC, 0, 0.5);  // throws where the reader kept no BEC evaluator
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const uint64_t b = std::strtoull(line.c_str(), nullptr, 16);
        double cap;
        std::memcpy(&cap, &b, 8);
        for (unsigned p = 0; p < l; ++p) {
            const double v = kern.GetSubchannelCapacity(ec_BEC, p, cap);
            uint64_t vb;
            std::memcpy(&vb, &v, 8);
            std::printf(p ? " %016llx" : "%016llx", (unsigned long long)vb);
        }
        std::putchar('\n');
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) return usage();
    try {
        const std::string mode = argv[1];
        if (mode == "decode" && argc == 4) return run_decode(argv[2], (unsigned)std::atoi(argv[3]));
        if (mode == "encode" && argc == 3) return run_encode(argv[2]);
        if (mode == "trellis" && argc == 3) return run_trellis(argv[2]);
        if (mode == "counts" && argc == 3) return run_counts(argv[2]);
        if (mode == "capacity" && argc == 3) return run_capacity(argv[2]);
        return usage();
    } catch (Exception &e) { /* the library's own (headers/external/misc.h:59) */
        std::fflush(stdout);
        std::fprintf(stderr, "polar_ref: %s\n", e.what());
        return 2;
    }
}
