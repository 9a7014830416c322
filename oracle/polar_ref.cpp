/* polar_ref.cpp -- TEST INFRASTRUCTURE ONLY. Our own driver around the reference's vendored
 * polar library (out/external/*.cpp, headers/external/*.h of the reference tree), linked by
 * oracle/Makefile into oracle/_ref/polar_ref together with eleven of that library's
 * translation units, read in place. It holds no text of the library. oracle/make_golden.py
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

/* Symbols the eleven translation units leave undefined: the kernel capacity tables
 * (CapacityEvaluator.cpp, which needs GSL's interpolation) and one generator call of the
 * channel simulator. None is on the encode, decode or trellis path, so anything that would
 * compute with them says its name and aborts; fixture generation never gets there.
 * TruncatedArikanKernel.cpp builds capacity tables of the library's built-in "G" and "A5"
 * kernels as global objects, so one AWGN constructor and the two destructors do run, at
 * start-up and at exit, in every process: those three are inert (they build and free
 * nothing) instead of aborting. */
#define POLAR_REF_STUB(name)                                               \
    do {                                                                   \
        std::fprintf(stderr, "polar_ref: stub reached: %s\n", name);       \
        std::abort();                                                      \
    } while (0)

CKernelCapacityEvaluator *LoadCapacityEvaluator(eChannel, unsigned, std::istream &) {
    POLAR_REF_STUB("LoadCapacityEvaluator");
}
CAWGNCapacityInterpolator::CAWGNCapacityInterpolator(unsigned size, std::istream &) : CKernelCapacityEvaluator(size) {
    POLAR_REF_STUB("CAWGNCapacityInterpolator(istream)");
}
CAWGNCapacityInterpolator::CAWGNCapacityInterpolator(unsigned size, unsigned, double *, double *)
    : CKernelCapacityEvaluator(size), m_NumOfCapPoints(0), m_pCapacities(nullptr), m_pPhysCapacities(nullptr),
      m_DoNotDelete(true), m_ppInterpolators(nullptr), m_ppAcceletators(nullptr) {}
CAWGNCapacityInterpolator::~CAWGNCapacityInterpolator() {}
double CAWGNCapacityInterpolator::GetSubchannelCapacity(double, unsigned) {
    POLAR_REF_STUB("CAWGNCapacityInterpolator::GetSubchannelCapacity");
}
CBECCapacityEvaluator::CBECCapacityEvaluator(unsigned size, std::istream &) : CKernelCapacityEvaluator(size) {
    POLAR_REF_STUB("CBECCapacityEvaluator(istream)");
}
CBECCapacityEvaluator::~CBECCapacityEvaluator() {}
double CBECCapacityEvaluator::GetSubchannelCapacity(double, unsigned) {
    POLAR_REF_STUB("CBECCapacityEvaluator::GetSubchannelCapacity");
}
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
    std::fprintf(stderr, "usage: polar_ref decode SPEC L | encode SPEC | trellis KERNEL  (rows on stdin)\n");
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

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) return usage();
    try {
        const std::string mode = argv[1];
        if (mode == "decode" && argc == 4) return run_decode(argv[2], (unsigned)std::atoi(argv[3]));
        if (mode == "encode" && argc == 3) return run_encode(argv[2]);
        if (mode == "trellis" && argc == 3) return run_trellis(argv[2]);
        return usage();
    } catch (Exception &e) { /* the library's own (headers/external/misc.h:59) */
        std::fflush(stdout);
        std::fprintf(stderr, "polar_ref: %s\n", e.what());
        return 2;
    }
}
