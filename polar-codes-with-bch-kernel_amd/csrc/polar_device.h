// polar_device.h -- what the host runtime (polar_host.cpp) shares with the gfx950 polar
// kernels: the parameter blocks, LDS layouts and save-slot format of the SC-list decoders
// (polar_sclist.hip, polar_sclist_q8.hip, polar_mixed.hip), the simulation front-end (polar_channel.hip) and
// genie-aided SC (polar_genie.hip). PolarIo opens both decoder parameter blocks. The device
// routines the kernels share are in polar_list_device.h (decisions, LoadLLRs),
// polar_llr_device.h (SoftXOR, mixed-kernel LLRs and partial sums) and polar_tier_device.h (the
// tiered kernels' index table). Plain C++, no HIP types.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bchk {

constexpr int kPolarMaxList = 32;    // 2 L candidates, one per lane of a wave
constexpr int kPolarMaxLayers = 14;  // U <= 2^14 (LDS bounds it further)

// The caller's buffers and the code's tables that every SC-list kernel reads and writes: the
// first member of both parameter blocks, filled once by the host (polar_host.cpp) and used by
// the kernels' LoadLLRs (plist::chan_llr) and epilogues.
struct PolarIo {
    const float *llr;       // [B][N] channel LLRs, log P(0)/P(1) (the decoder's reading)
    uint8_t *info;          // [B][L][K] information vectors, best path first
    uint8_t *cw;            // [B][L][N] codewords (may be null)
    float *metric;          // [B][L] path metrics
    int32_t *count;         // [B] list entries written
    const int16_t *symmap;  // [U] LoadLLRs: index into the LLR row; -1 shortened, -2 punctured
    const uint16_t *phase;  // [U] bit 0 frozen | (dynamic-freezing bit + 1) << 1 | has-correction << 8
    const uint64_t *dfcorr; // [U] dynamic-freezing correction masks
    const int16_t *cwpos;   // [N] transmitted (neither shortened nor punctured) symbols
};

// One SC-list decode launch: B codewords, one wave each, every path's arrays in LDS.
struct PolarParams {
    PolarIo io;
    uint32_t B;
    int32_t n, U, N, K, L;
    int32_t pathCw;                       // packed partial-sum words per path
    int32_t cwoff[kPolarMaxLayers + 1];   // word offset of C_λ in a path's packed array
};
// the kernel arguments keep their byte layout
static_assert(sizeof(PolarIo) == 72 && offsetof(PolarParams, B) == 72 && sizeof(PolarParams) == 160, "PolarParams layout");

constexpr uint16_t kPhaseFrozen = 1u, kPhaseCorr = 0x100u;


// (constexpr: usable from device code too.) Per-path strides in LDS, padded by 16 bytes so that the same element of consecutive paths
// falls in different banks (64 x 4 B banks): S holds U floats, C 3U bytes.
constexpr int polar_path_s(int U) { return ((U + 3) & ~3) + 4; }
constexpr int polar_path_c(int U) { return ((3 * U + 15) & ~15) + 16; }
constexpr int polar_rec_words(int K) { return K > 0 ? (K + 31) / 32 : 1; }

// Mixed kernels (polar_mixed.hip): layer j has a kernel of size ksize[j] (Arikan or a
// matrix, rows as 64-bit masks krows[j * kPolarMaxKernel + r], bit c = K[r][c]); outer[λ] =
// U / (ksize[0] ... ksize[λ-1]); per path S layer λ at soff[λ] (outer[λ] floats, λ >= 1), C
// layer λ at coff[λ] (outer[λ] ksize[λ-1] bytes, C_0 = U), matrix offset states at ooff[j].
constexpr int kPolarMaxKernel = 64;
constexpr int kPolarMaxMatrixGpu = 64;  // the 2^6 extended-BCH kernel (CTrellisKernelProcessor: < 64)
constexpr int kPolarMaxTrellisKernel = 32;  // the trellis is built for kernels up to 32 only
// Matrix layers of size > 32 (or from BCHK_POLAR_ML up) take their LLRs from an exact
// ordered-statistics search instead (one wave per item, polar_mixed.hip ml_llr): per wave an
// LDS scratch of kMlStack 12-byte search nodes, the reduced basis and the suffix unions of its
// non-pivot parts (64 + 65 u64), flip costs and |y| (64 floats each). Phases whose coset has
// at most 2^kMlEnumBits words are enumerated.
#ifndef BCHK_ML_STACK
#define BCHK_ML_STACK 768  // (64,32) L=8 2 dB, 8 192 words: 1536 nodes 950, 768 1 159, 512 1 116 codewords/s (profiles/r05_f4/ml_stack_variants.jsonl)
#endif
constexpr int kMlStack = BCHK_ML_STACK;
constexpr int kMlEnumBits = 10;
// The scratch's carve-up (polar_mixed.hip MlScratch), each array where the one before ends:
// G at 0, then
constexpr uint32_t kMlOffU = 8u * 64u;                    // past G [64] u64
constexpr uint32_t kMlOffCost = kMlOffU + 8u * 65u + 8u;  // past U [65] u64 and 8 bytes of padding
constexpr uint32_t kMlOffAy = kMlOffCost + 4u * 64u;      // past cost [64] f32
// the scratch before the stack (G, U, cost, ay), saved with a suspended search together with
// the stack's live nodes
constexpr uint32_t kMlHeadBytes = kMlOffAy + 4u * 64u;    // past ay [64] f32: the stack
constexpr uint32_t kMlNodeBytes = 12u;                    // sizeof(MlNode)
constexpr uint32_t kMlScratchBytes = kMlHeadBytes + kMlNodeBytes * kMlStack;
// u64 arrays on 8 bytes; a save slot takes the head and the live nodes as 32-bit words
static_assert(kMlOffU % 8 == 0 && kMlHeadBytes % 4 == 0 && kMlNodeBytes % 4 == 0, "search scratch alignment");
// Matrix layers of size >= the trellis threshold (default 16, BCHK_POLAR_TRELLIS) take their
// LLRs from CTrellisKernelProcessor's trellis (pull-form Viterbi over predecessor lists);
// smaller ones enumerate the coset (2^(size - 1 - phase) words per LLR). Per (layer, phase):
// tlog[(layer * kPolarMaxKernel + phase) * (kPolarMaxKernel + 1) + d] = log2 of the states at
// depth d (d = 0..size), tbase[layer * kPolarMaxKernel + phase] = first entry of the phase in
// tent; entries run depth by depth, one per state of depth d + 1, two 16-bit predecessors
// (state | z << 13 | valid << 14).
constexpr int kPolarTrellisMaxBits = 12;
constexpr uint32_t kTrellisZ = 1u << 13, kTrellisValid = 1u << 14, kTrellisState = kTrellisZ - 1u;
// The named kernels "G" (3 x 3) and "A5" (5 x 5) of TruncatedArikanKernel.cpp are matrix layers
// for the encoder and the partial sums (their rows), but take their LLRs from the library's
// own recursive f/g processors (pllr::named_llrs), which keep a state per path and element
// from one phase to the next: G one float (L1 [+] L2) at foff[j] + s; A5 three floats L04, L13,
// L024 at foff[j] + {0, d, 2d} + s (d = outer[j + 1]) and one bit at ooff[j] + s. The floats
// lie in the path's S stride past its layers, the bit in its offset-state stride: what a path
// clone copies and a save slot covers.
constexpr uint8_t kNamedG = 1, kNamedA5 = 2;
constexpr int polar_named_floats(int kind) { return kind == kNamedG ? 1 : kind == kNamedA5 ? 3 : 0; }
struct PolarMixedParams {
    PolarIo io;
    const uint64_t *krows;  // [nl][kPolarMaxKernel]
    const uint32_t *tent, *tbase;  // trellis predecessor lists (see above)
    const uint8_t *tlog;
    int32_t tstates;               // largest state count of any trellis layer (>= 64 if any)
    uint32_t B;
    int32_t nl, U, N, K, L;
    int32_t ssize, csize, osize;
    int32_t ksize[kPolarMaxLayers], outer[kPolarMaxLayers + 1];
    int32_t soff[kPolarMaxLayers + 1], coff[kPolarMaxLayers + 1], ooff[kPolarMaxLayers];
    uint8_t arikan[kPolarMaxLayers];
    uint8_t trellis[kPolarMaxLayers];  // matrix layer decoded through its trellis
    uint8_t ml[kPolarMaxLayers];       // matrix layer decoded by the ordered-statistics search
    uint8_t named[kPolarMaxLayers];    // kNamedG / kNamedA5: the f/g processor of a named kernel
    int32_t foff[kPolarMaxLayers];     // a named layer's float state in the path's S stride
    int32_t any_ml;                    // LDS holds the search scratch
    // Time-budgeted launches (round 6; codes with search layers): a wave past `budget` ticks
    // of the 100 MHz clock since its launch began suspends its codeword between two search
    // items (its LDS state and registers to rsave, rstate[cw] = 1) and starts no other; the
    // host launches again until `unfinished` stays 0. rstate: 0 not started, 1 suspended,
    // 2 done. budget 0 (or rstate null): every codeword runs to its end in one launch.
    // A wave always starts (or resumes) the first unfinished codeword it meets in a launch,
    // whatever the clock says, and a search runs at least one round per launch: every launch
    // that leaves codewords unfinished has done work (`progress` > 0), however small the budget.
    // A wave has at most one suspended codeword -- after suspending it starts nothing more, and
    // the next launch (same grid) resumes it before anything else -- so rsave holds one slot
    // per workgroup, not per codeword.
    uint32_t *rstate;
    uint8_t *rsave;         // [grid][rstride]
    uint32_t rstride;       // bytes of rsave per workgroup (PolarMixedLayout::save_bytes)
    uint32_t *unfinished;   // codewords left suspended or not started by this launch
    uint32_t *progress;     // search rounds (at least), items and codewords completed by this launch
    uint64_t budget;
    int32_t no_mid;         // experiments: suspend between search items only (BCHK_POLAR_NO_MID)
    uint32_t ml_rounds;     // a search past this many rounds in all gives NaN (BCHK_POLAR_ML_ROUNDS)
};
constexpr uint32_t kMlRoundsDefault = 1u << 20;
static_assert(offsetof(PolarMixedParams, krows) == 72 && sizeof(PolarMixedParams) == 608, "PolarMixedParams layout");

// A suspended codeword's save slot (PolarMixedParams::rsave): the header, six registers per
// lane, then the LDS of the list state -- channel / S / C / O ([0, o_ph)) at kSaveLdsOff,
// act / rec ([o_act, o_tm)) at sv_act -- and at sv_ml a suspended search's scratch (its head
// and live nodes; room for kMlScratchBytes).
struct PolarSaveHeader {      // (32-bit words 0..14 of the slot)
    uint32_t phi, layer, item;  // where to resume: phase, layer of its LLR recursion, search item
    uint32_t k, active, top;    // unfrozen decisions so far, active paths, the path stack's top
    uint32_t mid;               // suspended inside a search item: the fields below and the scratch
    uint32_t sp;                // MlResume (polar_mixed.hip): live stack nodes,
    float best0, best1;
    uint64_t hd, lrb;
    uint32_t rounds;
};
struct PolarSaveLane {        // lane q: path q's scalars and slot q of the path stack
    float R, lv;
    uint64_t dm;
    uint32_t rw, slot;
};
constexpr uint32_t kSaveHeaderBytes = 64, kSaveLaneBytes = 24;
constexpr uint32_t kSaveLdsOff = kSaveHeaderBytes + 64u * kSaveLaneBytes;
static_assert(sizeof(PolarSaveHeader) <= kSaveHeaderBytes && sizeof(PolarSaveLane) == kSaveLaneBytes, "save slot");

// The kernel's LDS offsets (polar_mixed.hip) and size, and the save slot's: channel, per path
// S / C / offset states, phases, kernel rows, act / rec, the trellis state metrics (two
// buffers of tstates floats) and, with a search layer (ml), the search scratch.
struct PolarMixedLayout {
    int o_S, o_C, o_O, o_ph, o_rows, o_act, o_tm, o_ml;
    uint32_t bytes;
    uint32_t sv_act, sv_ml, save_bytes;
};
__host__ __device__ inline PolarMixedLayout polar_mixed_layout(int U, int L, int K, int ssize, int csize, int osize,
                                                               int nl, int tstates, bool ml) {
    PolarMixedLayout o;
    o.o_S = (4 * U + 15) & ~15;
    o.o_C = o.o_S + 4 * ssize * L;
    o.o_O = o.o_C + csize * L;
    o.o_ph = (o.o_O + osize * L + 15) & ~15;
    o.o_rows = (o.o_ph + 2 * U + 15) & ~15;
    o.o_act = o.o_rows + 8 * kPolarMaxKernel * nl;
    o.o_tm = (o.o_act + 4 * L + 4 * L * polar_rec_words(K) + 15) & ~15;
    o.o_ml = (o.o_tm + 8 * tstates + 15) & ~15;
    o.bytes = ((uint32_t)o.o_ml + (ml ? kMlScratchBytes : 0u) + 15u) & ~15u;
    o.sv_act = kSaveLdsOff + (uint32_t)o.o_ph;
    o.sv_ml = o.sv_act + (uint32_t)(o.o_tm - o.o_act);
    o.save_bytes = (o.sv_ml + kMlScratchBytes + 15u) & ~15u;
    return o;
}

// ---- the simulation front-end (polar_channel.hip): encoder, AWGN LLRs, error counters.
// The encoder's tables (device pointers into the context's blob): u is built from the
// information bits (inforank), the dynamic freezing constraints in symbol order (static ones
// are zeros), then the layers' transform, innermost first, and the transmitted symbols.
struct PolarEncTables {
    const int16_t *inforank;  // [U] index of the symbol among the unfrozen ones, -1 = frozen
    const int16_t *cwpos;     // [N] transmitted symbols
    const uint64_t *krows;    // [nl][kPolarMaxKernel]
    const uint32_t *dynoff;   // [ndyn + 1] first term of dynamic constraint d in dynterm
    const uint16_t *dynterm;  // terms, ascending, the frozen symbol last
    int32_t ndyn, nl, U, N, K;
    int32_t ksize[kPolarMaxLayers];
};
// One launch over B words: an encode (info_in -> cw) or, with gen set, words
// [word0, word0 + B) of the counter-based stream (bchk_philox.h): information bits, codeword,
// LLR = (float)(-2 y / var), y = BPSK(bit 1 -> +1) + sigma z in double. The channel
// (BCHK_CHANNEL_*, include/bchk.h) chooses the kernel's instantiation: Rayleigh fades x by
// h = sqrt(-log u) and weighs the LLR with it, the BSC flips x where u <= cross and stores -2 y.
constexpr int kPolarChanAwgn = 0, kPolarChanRayleigh = 1, kPolarChanBsc = 2;
// The fading models with a parameter (BCHK_FADING_* + kPolarChanFading, the *_fading entry
// points): y = h x + sigma z and LLR = ((-2 h) y) / var as on the Rayleigh channel, with
//   block:      h = the Rayleigh factor of the first element of the position's block of fblock
//   correlated: h_q = sqrt((a_q^2 + b_q^2) / 2) on elements 2 q, 2 q + 1 of the word; a, b two
//               AR(1) sequences g_0 = z_0, g_q = fma(f0, g_{q-1}, f1 z_q) over the normal pairs
//               of counter (word low, word high, kTagCorrelated, q): f0 = rho, f1 = sqrt(1 - rho^2)
//   Rician:     h = sqrt((f0 + f1 z1)^2 + (f1 z2)^2), (z1, z2) the normal pair of counter (word
//               low, word high, kTagRician, position): f0 = v, f1 = s
constexpr int kPolarChanFading = 3;
constexpr int kPolarChanBlock = 3, kPolarChanCorrelated = 4, kPolarChanRician = 5;
struct PolarGenParams {
    PolarEncTables t;
    const uint8_t *info_in;  // [B][K] (encode)
    uint8_t *info;           // [B][K] (generate; may be null)
    uint8_t *cw;             // [B][N] (may be null when generating)
    float *llr;              // [B][N] (generate)
    uint64_t word0;
    uint32_t B;
    uint32_t seed_lo, seed_hi;
    int32_t gen;
    double sigma, var;
    int32_t channel;         // kPolarChan*
    double cross;            // the BSC's crossover probability
    int32_t fblock;          // block fading: the block size, 1 .. N
    double f0, f1;           // correlated and Rician fading: see above
    double *fade;            // [B][N] h (Rayleigh and the fading models; may be null)
    double *y;               // [B][N] the channel output before the demodulator (may be null)
};
// CSimulator::Iterate's counters of one decoded batch (Simulator.cpp:201-318), added into
// out8: words, block errors, information bit errors, code bit errors, ML errors, list errors,
// raw bit errors, words with count <= 0.
struct PolarCountParams {
    const uint8_t *info_tx, *cw_tx;  // [B][K], [B][N] sent
    const float *llr;                // [B][N]
    const uint8_t *info, *cw;        // [B][L][K], [B][L][N] decoded lists
    const int32_t *count;            // [B]
    unsigned long long *out8;
    uint8_t *flags;                  // [B] bit 0 block, 1 ML, 2 list error (may be null)
    uint32_t B;
    int32_t N, K, L;
};
constexpr int kPolarChanWaves = 4;  // waves per workgroup of both kernels, one word per wave
// LDS bytes of one wave of the generate / encode kernel: the packed information bits (whole
// 128-bit generator blocks) and two packed buffers of u (the layers ping-pong)
constexpr uint32_t polar_gen_wave_bytes(int U, int K) {
    return 8u * (uint32_t)(2 * ((K + 127) / 128) + 2) + 16u * (uint32_t)((U + 63) / 64);
}

// ---- genie-aided SC (polar_genie.hip): one path per word in the mixed layout above (every
// code, all-Arikan ones included), fed back with the sent u instead of its decisions. The
// kernel writes per word the U decision LLRs and the U rebuilt encoder inputs as rows; a second
// kernel sums the columns into the per-symbol error counts and soft sums (integers: the result
// does not depend on grids, batch splits or the order of waves).
struct PolarGenieParams {
    PolarEncTables t;        // u is rebuilt as polar_gen_kernel does (polar_enc_device.h)
    const uint8_t *info_tx;  // [B][K] sent information bits
    const float *llr;        // [B][N] channel LLRs
    float *dec_llr;          // [B][U] decision LLRs (rows)
    uint8_t *u;              // [B][U] encoder inputs (rows)
    const int16_t *symmap;   // [U] LoadLLRs
    const uint32_t *tent, *tbase;  // trellis tables (PolarMixedParams)
    const uint8_t *tlog;
    int32_t tstates;
    uint32_t B;
    int32_t ssize, csize, osize;
    int32_t outer[kPolarMaxLayers + 1];
    int32_t soff[kPolarMaxLayers + 1], coff[kPolarMaxLayers + 1], ooff[kPolarMaxLayers];
    uint8_t arikan[kPolarMaxLayers], trellis[kPolarMaxLayers];
    uint8_t named[kPolarMaxLayers];  // as in PolarMixedParams
    int32_t foff[kPolarMaxLayers];
};
// LDS of one wave: channel LLRs, S, C, offset states, kernel rows, the trellis metric buffers
// (2 x tstates floats), the packed information bits and the packed u
struct PolarGenieLayout {
    int o_S, o_C, o_O, o_rows, o_tm, o_ib, o_u;
    uint32_t bytes;
};
__host__ __device__ inline PolarGenieLayout polar_genie_layout(int U, int K, int ssize, int csize, int osize, int nl,
                                                               int tstates) {
    PolarGenieLayout o;
    o.o_S = (4 * U + 15) & ~15;
    o.o_C = o.o_S + 4 * ssize;
    o.o_O = o.o_C + csize;
    o.o_rows = (o.o_O + osize + 15) & ~15;
    o.o_tm = o.o_rows + 8 * kPolarMaxKernel * nl;
    o.o_ib = o.o_tm + 8 * tstates;
    o.o_u = o.o_ib + 8 * (2 * ((K + 127) / 128) + 2);
    o.bytes = (uint32_t)((o.o_u + 8 * ((U + 63) / 64) + 15) & ~15);
    return o;
}
// words of one launch a workgroup of the column-sum kernel covers for its 64 symbols
constexpr uint32_t kGenieSumRows = 32;

// Packed partial sums of the all-Arikan kernel (polar_sclist.hip): per path C_0 (U bits,
// the codeword) then C_λ (U >> (λ-1) bits, λ = 1..n), each starting on a 32-bit word; the
// path stride is odd, so the same word of different paths falls in different banks. Writes
// the word offsets (n + 1 entries) when off is given; returns the stride in words.
inline int polar_cw_layout(int U, int32_t *off) {
    int n = 0;
    while ((1 << n) < U) ++n;
    int w = 0;
    for (int lam = 0; lam <= n; ++lam) {
        if (off) off[lam] = w;
        const int bits = lam == 0 ? U : (U >> (lam - 1));
        w += (bits + 31) / 32;
    }
    return w | 1;
}

// LDS of one wave's state (see polar_sclist.hip): per path S (floats, at 0) and the packed
// partial sums (pathCw = polar_cw_layout's stride), the active-path list and right after it
// per path the information bits decided so far. The channel LLRs and the phase table are read
// from global memory (layer 0 is read at two phases per codeword, the phase word once per phase).
struct PolarListLayout {
    int o_C, o_act;
    uint32_t bytes;
};
__host__ __device__ inline PolarListLayout polar_list_layout(int U, int L, int K, int pathCw) {
    PolarListLayout o;
    o.o_C = 4 * polar_path_s(U) * L;
    o.o_act = (o.o_C + 4 * pathCw * L + 15) & ~15;
    o.bytes = (uint32_t)((o.o_act + 4 * L + 4 * L * polar_rec_words(K) + 15) & ~15);
    return o;
}

// ---- the fixed-point all-Arikan kernel (polar_sclist_q8.hip): polar_sclist_kernel with int8
// LLRs (the arithmetic contract: include/bchk.h). The block opens with PolarParams
// and so with PolarIo: the map of LoadLLRs, the phase table and the output buffers are the f32
// kernel's; io.llr is not read, the rows come from llr8.
struct PolarQ8Params {
    PolarParams p;
    const int8_t *llr8;  // [B][N] channel LLRs, negative favours 1; -128 reads as -127
};
static_assert(offsetof(PolarQ8Params, llr8) == 160 && sizeof(PolarQ8Params) == 168, "PolarQ8Params layout");
constexpr int kQ8Max = 127;  // the symmetric saturation bound; a shortened symbol's LLR

// Per path S holds the U - 1 LLRs of the layers 1..n as bytes, layer λ at U - (U >> (λ-1)) as in
// the f32 kernel: whole 16-byte pieces for the clone copy, and 16 bytes of padding, so that the
// same word of consecutive paths falls in banks 4 apart. C, act and rec are polar_list_layout's.
constexpr int polar_path_q8(int U) { return ((U + 15) & ~15) + 16; }
__host__ __device__ inline PolarListLayout polar_q8_layout(int U, int L, int K, int pathCw) {
    PolarListLayout o;
    o.o_C = polar_path_q8(U) * L;
    o.o_act = (o.o_C + 4 * pathCw * L + 15) & ~15;
    o.bytes = (uint32_t)((o.o_act + 4 * L + 4 * L * polar_rec_words(K) + 15) & ~15);
    return o;
}

// ---- the tiered all-Arikan kernel (polar_sclist_tiered.hip): S_λ and C_λ of the layers
// λ <= split, and C_0, live in a per-workgroup workspace in global memory; the layers below the
// split stay in LDS in polar_list_layout's form for the sub-code of length U >> split.
struct PolarTieredParams {
    PolarParams p;
    uint8_t *ws;         // [grid][ws_bytes] (PolarTieredLayout)
    int32_t split;
    int32_t cwsplit;     // packed words of C_0 .. C_split: cwoff[split + 1], or all of them at split = n
    int32_t cwall;       // packed words of C_0 .. C_n
};
// words of the packed C_λ (polar_cw_layout: U bits at λ = 0, U >> (λ-1) after, whole words)
constexpr int polar_cw_words(int U, int lam) {
    return lam == 0 ? ((U + 31) >> 5) : (((U >> (lam - 1)) + 31) >> 5);
}
// LDS: per path the S layers split+1 .. n (floats, at 0; layer λ at (U >> split) - (U >> (λ-1)))
// and their packed C (word cwoff[λ] - cwsplit of the path's pathC words), the global layers'
// array index of every path (idx[(λ-1) L + q], bytes) and one array-owner byte per array, then
// act / rec as in PolarListLayout.
// Workspace of one workgroup: per global layer λ = 1..split L arrays of U >> λ floats, layer λ at
// float L (U - (U >> (λ-1))); at w_C, L arrays per packed layer, layer λ at word L cwoff[λ]
// (C_0's arrays belong to the paths, the others are shared through idx).
struct PolarTieredLayout {
    int pathS, pathC, n_C;  // LDS strides per path (floats -- bytes in the q8 layout --, words) and the C words in use
    int o_C, o_idx, o_own, o_act;
    uint32_t bytes;
    uint64_t w_C, ws_bytes;
};
__host__ __device__ inline PolarTieredLayout polar_tiered_layout(int U, int L, int K, int split, int cwsplit,
                                                                 int cwall) {
    PolarTieredLayout o;
    const int Us = U >> split;  // 1 at split = n: nothing of S or C in LDS
    o.pathS = Us > 1 ? polar_path_s(Us) : 0;
    o.n_C = cwall - cwsplit;
    o.pathC = o.n_C ? (o.n_C | 1) : 0;
    o.o_C = 4 * o.pathS * L;
    o.o_idx = o.o_C + 4 * o.pathC * L;
    o.o_own = o.o_idx + split * L;
    o.o_act = (o.o_own + L + 15) & ~15;
    o.bytes = (uint32_t)((o.o_act + 4 * L + 4 * L * polar_rec_words(K) + 15) & ~15);
    o.w_C = (4ull * (uint64_t)L * (uint64_t)(U - Us) + 15ull) & ~15ull;
    o.ws_bytes = (o.w_C + 4ull * (uint64_t)L * (uint64_t)cwsplit + 255ull) & ~255ull;
    return o;
}

// ---- the tiered fixed-point all-Arikan kernel (polar_sclist_q8_tiered.hip): the tiered kernel
// with the int8 LLRs of polar_sclist_q8.hip. The block opens with
// PolarTieredParams; io.llr is not read, the rows come from llr8.
struct PolarQ8TieredParams {
    PolarTieredParams t;
    const int8_t *llr8;  // [B][N] channel LLRs, as PolarQ8Params::llr8
};
static_assert(offsetof(PolarTieredParams, ws) == 160 && offsetof(PolarTieredParams, split) == 168 &&
                  offsetof(PolarQ8TieredParams, llr8) == 184 && sizeof(PolarQ8TieredParams) == 192,
              "PolarQ8TieredParams layout");
// polar_tiered_layout with byte LLRs (pathS counts bytes here). LDS: per path the S layers
// split+1 .. n in polar_path_q8's form for the sub-code, layer λ at byte (U >> split) - (U >> (λ-1));
// C, idx, own, act and rec as in the f32 tiered layout.
// Workspace of one workgroup: per global layer λ = 1..split L arrays of U >> λ bytes, layer λ at
// byte L (U - (U >> (λ-1))) -- so an array of at least 4 bytes starts on a dword and one of at
// least 16 on 16 -- and at w_C the packed C arrays exactly as the f32 tiered kernel has them.
__host__ __device__ inline PolarTieredLayout polar_q8_tiered_layout(int U, int L, int K, int split, int cwsplit,
                                                                    int cwall) {
    PolarTieredLayout o;
    const int Us = U >> split;
    o.pathS = Us > 1 ? polar_path_q8(Us) : 0;
    o.n_C = cwall - cwsplit;
    o.pathC = o.n_C ? (o.n_C | 1) : 0;
    o.o_C = o.pathS * L;
    o.o_idx = o.o_C + 4 * o.pathC * L;
    o.o_own = o.o_idx + split * L;
    o.o_act = (o.o_own + L + 15) & ~15;
    o.bytes = (uint32_t)((o.o_act + 4 * L + 4 * L * polar_rec_words(K) + 15) & ~15);
    o.w_C = ((uint64_t)L * (uint64_t)(U - Us) + 15ull) & ~15ull;
    o.ws_bytes = (o.w_C + 4ull * (uint64_t)L * (uint64_t)cwsplit + 255ull) & ~255ull;
    return o;
}

// ---- the tiered mixed-kernel decoder (polar_mixed_tiered.hip): polar_mixed_kernel with the
// state of the layers j < split of every path in a per-workgroup workspace in global memory.
// Layer j's group is what its LLR step and the partial sums of its blocks write: S_{j+1}, the
// named layer's floats F_j, C_{j+1} and the offset state O_j. Per group there are L arrays,
// shared between the paths through an index table in LDS (Tal and Vardy's lazy copy, as in the
// tiered all-Arikan kernel); C_0 (one array per path) and the mapped channel LLRs lie there too.
// The layers j >= split keep the mixed layout for the inner sub-code in LDS.
// In `m` the per-layer offsets mean, for a global layer j < split, places in one array of its
// group: S_{j+1} at 0, F_j at float foff[j], C_{j+1} at byte coff[j + 1], O_j at byte ooff[j];
// for j >= split, places in the path's LDS strides ssize / csize / osize as in PolarMixedParams
// (soff[j + 1] and foff[j] floats, coff[j + 1] and ooff[j] bytes). Search layers (ml) are not taken.
struct PolarMixedTieredParams {
    PolarMixedParams m;
    uint8_t *ws;                        // [grid][ws_bytes] (PolarMixedTieredLayout)
    int32_t split;
    int32_t garr[kPolarMaxLayers];      // bytes of one array of group j
    int32_t gbase[kPolarMaxLayers];     // first array of group j, bytes past w_grp (L arrays each)
    int32_t gobytes[kPolarMaxLayers];   // bytes of O_j, and
    int32_t gfloats[kPolarMaxLayers];   // floats of F_j, in an array of group j
    int32_t grp_bytes;                  // all groups' arrays: the sum of L garr[j], j < split
};
// LDS: per path S / C / O of the inner layers, the groups' array index of every path
// (idx[j L + q], bytes) and one array-owner byte per array, then phases, kernel rows, act / rec
// and the trellis metric buffers as in PolarMixedLayout.
// Workspace of one workgroup: the channel LLRs after LoadLLRs (U floats), C_0 of every path (L
// arrays of c0 bytes), then the groups' arrays.
struct PolarMixedTieredLayout {
    int o_C, o_O, o_idx, o_own, o_ph, o_rows, o_act, o_tm;  // (S at 0)
    uint32_t bytes;
    uint32_t c0, w_C0, w_grp;
    uint64_t ws_bytes;
};
__host__ __device__ inline PolarMixedTieredLayout polar_mixed_tiered_layout(int U, int L, int K, int ssize, int csize,
                                                                            int osize, int nl, int split, int tstates,
                                                                            int grp_bytes) {
    PolarMixedTieredLayout o;
    o.o_C = 4 * ssize * L;
    o.o_O = o.o_C + csize * L;
    o.o_idx = o.o_O + osize * L;
    o.o_own = o.o_idx + split * L;
    o.o_ph = (o.o_own + L + 15) & ~15;
    o.o_rows = (o.o_ph + 2 * U + 15) & ~15;
    o.o_act = o.o_rows + 8 * kPolarMaxKernel * nl;
    o.o_tm = (o.o_act + 4 * L + 4 * L * polar_rec_words(K) + 15) & ~15;
    o.bytes = (uint32_t)((o.o_tm + 8 * tstates + 15) & ~15);
    o.c0 = ((uint32_t)U + 15u) & ~15u;
    o.w_C0 = (4u * (uint32_t)U + 15u) & ~15u;
    o.w_grp = o.w_C0 + (uint32_t)L * o.c0;
    o.ws_bytes = ((uint64_t)o.w_grp + (uint64_t)grp_bytes + 255ull) & ~255ull;
    return o;
}

}  // namespace bchk
