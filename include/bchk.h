/* include/bchk.h -- C ABI of libbchk.so, the MI355X (gfx950) Kaneko/BCH soft decoder.
 *
 * This is the drop-in boundary for the reference's hot path. The reference has no FFI;
 * its boundary is the C++ class API below, which the headers in include/bchk_dropin/ re-declare
 * on top of these entry points. Each entry point names the
 * reference interface it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *  - Every function returns 0 on success and a negative BCHK_E* code on failure;
 *    bchk_last_error() describes the last failure of the calling thread. Nothing throws.
 *  - One context = one (code, J, decoder SNR, device); it owns a HIP stream. A context
 *    is not thread-safe; use one per host thread. It also owns the work queues, control
 *    words and fused-counter slots of its decode calls: at most ONE decode call per
 *    context may be in flight on the device at a time. Calls enqueued on the same stream
 *    serialise by themselves; a caller that passes different streams to consecutive calls
 *    must order them (an event, or bchk_sync) -- otherwise one call's counter reduction
 *    can fold and zero the other's partial counts. Use one context per concurrent stream.
 *  - Kernels never hang on a work-queue wait: every wait is bounded, and a wait that runs
 *    out leaves its codeword unfinished and sets the context's fault word. bchk_sync (and
 *    every synchronous *_host call) then fails with BCHK_EHIP and clears it.
 *  - Bit vectors are one byte per position (0/1), position i = coefficient of x^i,
 *    exactly as the reference's unsigned char arrays.
 *  - *_host functions take host pointers and are synchronous. *_device functions take
 *    device pointers, enqueue on `stream` (a hipStream_t, NULL = the context's stream)
 *    and return immediately.
 *  - There is NO CPU fallback: without a usable gfx950 device every compute call fails
 *    with BCHK_ENODEV.
 */
#ifndef BCHK_H
#define BCHK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCHK_OK 0
#define BCHK_EINVAL -1   /* bad argument / unsupported (m, t)                       */
#define BCHK_ENODEV -2   /* no HIP device, or the gfx950 code object failed to load */
#define BCHK_EHIP -3     /* a HIP runtime call failed                               */
#define BCHK_ENOMEM -4

/* J: the reference's test-pattern exponent cap.
 *   BCHK_J_SHIPPED (-1): as shipped, `T = j` (src/KanekoKernelProcessor.cpp:393);
 *   J >= 0: the commented-out `T = (j > J) ? J : j` (:392, J = 15 in the header :35). */
#define BCHK_J_SHIPPED (-1)

/* Decoder variants of KanekoKernelProcessor::decode */
#define BCHK_VARIANT_ANSWER 0 /* decode(answer, word, res) :335-407 (used by fun())       */
#define BCHK_VARIANT_WORD 1   /* decode(word, res)         :212-276 (main.cpp file mode)  */

/* per-codeword flags (bchk_stats.flags) */
#define BCHK_F_ACCEPTED 1u   /* res was written (else the row is left untouched)       */
#define BCHK_F_RETURNED 2u   /* left through `l < calcRightSide()` (:380-382)          */
#define BCHK_F_TRUNCATED 4u  /* stopped at the context's max_decodes safety cap:        */
                             /* result is NOT the reference's                           */
#define BCHK_F_TIE 8u        /* two |alpha| exactly equal: std::sort order unspecified  */
#define BCHK_F_SCAN_UB 16u   /* VARIANT_WORD only: the unbounded calcT scan (:257)      */
                             /* would read past alphaSorted[n-1] (UB in the reference)  */

typedef struct bchk_stats {
    uint64_t decodes;      /* += decodingCount                                (:368) */
    uint64_t comparisons;  /* += comparisonCount                       (:387,396,402) */
    uint64_t sums;         /* += summCount                                 (:388,403) */
    uint64_t iterations;   /* completed loop iterations                               */
    uint64_t jsteps;       /* calcT scan steps                                        */
    uint64_t improvements; /* accepted candidates that did not return                 */
    uint32_t flags;        /* BCHK_F_*                                                */
    uint32_t reserved;
} bchk_stats;

typedef struct bchk_ctx bchk_ctx;

/* Replaces KanekoKernelProcessor::KanekoKernelProcessor(pw, n, t, k, antilog, log, snr)
 * (headers/KanekoKernelProcessor.h:47-50, src/KanekoKernelProcessor.cpp:17-26) plus the
 * GF/generator setup of src/main.cpp:59-93. Supported: 2 <= m <= 8, 1 <= t <= 32,
 * t < 2^(m-1) (main.cpp:55). decoder_snr_db is 0.5 in every reference call site. */
int bchk_create(int m, int t, int J, double decoder_snr_db, int device, bchk_ctx **out);
void bchk_destroy(bchk_ctx *ctx);

/* n, k (= n - deg g, main.cpp:93) and deg g + 1. */
int bchk_code_params(const bchk_ctx *ctx, int *n, int *k, int *gsize);
/* g(x) coefficients low -> high (gsize bytes), as printVec(g, gSize) in main.cpp:95. */
int bchk_generator(const bchk_ctx *ctx, uint8_t *g);
/* Safety cap on algebraic decodes per codeword (0 = unlimited, the default). Codewords
 * that hit it are flagged BCHK_F_TRUNCATED. */
int bchk_set_max_decodes(bchk_ctx *ctx, uint64_t max_decodes);

/* Replaces KanekoKernelProcessor::decode(answer, word, res)
 * (headers/KanekoKernelProcessor.h:55, src/KanekoKernelProcessor.cpp:335-407), batched:
 *   y   [B][n] channel samples (double), row b = `word` of codeword b
 *   res [B][n] decoded words; row b is written only if flags & BCHK_F_ACCEPTED
 *   l0  [B]    path metric of res (calcL(res)), DBL_MAX if not accepted   (may be NULL)
 *   st  [B]    counters / flags                                           (may be NULL)
 * `answer` is not an input: the reference ignores it (:345 computes an unused value). */
int bchk_decode_host(bchk_ctx *ctx, const double *y, size_t B, uint8_t *res, double *l0,
                     bchk_stats *st);
int bchk_decode_device(bchk_ctx *ctx, const double *d_y, size_t B, uint8_t *d_res,
                       double *d_l0, bchk_stats *d_st, void *stream);
/* As above for another decode() variant (BCHK_VARIANT_*). */
int bchk_decode_variant_host(bchk_ctx *ctx, int variant, const double *y, size_t B,
                             uint8_t *res, double *l0, bchk_stats *st);

/* Replaces Decoder::decode(word, answer) (headers/Decoder.h:78, src/Decoder.cpp:298-321),
 * batched. The reference decodes from its stored syndrome (findSyndromPoly/
 * alterSyndromPoly, src/Decoder.cpp:184-230) and flips bits of `word`; syndromes (may be
 * NULL) carries that stored state as the t odd syndromes S_1, S_3, ..., S_{2t-1} per word
 * ([N][t] GF elements as uint32). NULL = syndromes of `words` themselves.
 *   ok [N] 1 on success; answers [N][n] written only where ok. */
int bchk_alg_decode_host(bchk_ctx *ctx, const uint8_t *words, const uint32_t *syndromes,
                         size_t N, uint8_t *answers, uint8_t *ok);

/* FER/BER/op-counter accumulation of one batch (src/dataForPlot.cpp:55-74), on device:
 *   out6 += {frame errors, bit errors, decodes, comparisons, sums, words}
 * tx/res [B][n]; st [B] from bchk_decode_device. d_out6 is a device uint64_t[6]. */
int bchk_count_device(bchk_ctx *ctx, const uint8_t *d_tx, const uint8_t *d_res,
                      const bchk_stats *d_st, size_t B, uint64_t *d_out6, void *stream);
/* bchk_decode_device and bchk_count_device in one pass (the body of the reference's fun()
 * loop over a batch, src/dataForPlot.cpp:55-74): every kernel that finishes a codeword
 * compares its row with tx and adds to the counters, so res and st are not read back.
 *   d_st may be NULL (then no per-codeword stats are stored; the counters still include
 *   decodes, comparisons and sums); out6 += {frame errors, bit errors, decodes,
 *   comparisons, sums, words}. Rows never accepted keep the caller's contents and are
 *   counted as such, exactly as bchk_count_device after bchk_decode_device. */
int bchk_decode_count_device(bchk_ctx *ctx, const double *d_y, const uint8_t *d_tx, size_t B, uint8_t *d_res,
                             double *d_l0, bchk_stats *d_st, uint64_t *d_out6, void *stream);

/* The reference's input stream (src/bchCoder.cpp:228-250 in fun() order): minstd_rand0
 * seeded with `seed`, B words at Eb/N0 snr_db: tx [B][n], y [B][n]. rng_state (in/out,
 * may be NULL) is the engine state: pass 0 to start from `seed`. Host-side, sequential. */
int bchk_generate_host(const bchk_ctx *ctx, double snr_db, size_t B, uint64_t *rng_state,
                       uint64_t seed, uint8_t *tx, double *y);
/* As above, and draws = the engine draws the B words consumed. */
int bchk_generate_host_draws(const bchk_ctx *ctx, double snr_db, size_t B, uint64_t *rng_state,
                             uint64_t seed, uint8_t *tx, double *y, uint64_t *draws);
/* The engine state `draws` draws after `state` (minstd_rand0: state * 16807^draws mod
 * 2^31 - 1; a seed is a state): disjoint ranges of the one reference stream per rank or
 * process. */
uint64_t bchk_rng_jump(uint64_t state, uint64_t draws);
/* One block of a (sharded) fun() sweep (src/dataForPlot.cpp:41-74): from engine state
 * *rng_state (in/out), `skip` words are passed over (their engine draws only, no samples),
 * then B words are generated at Eb/N0 snr_db and decoded on the GPU:
 *   tx [B][n], res [B][n] (zero where not accepted), accepted [B], ops [B][3] = decodes,
 *   comparisons, sums, states [B] = engine state after word b (where a sweep resumes when
 *   it stops after word b). */
int bchk_sweep_block(bchk_ctx *ctx, double snr_db, uint64_t *rng_state, size_t skip, size_t B,
                     uint8_t *tx, uint8_t *res, uint8_t *accepted, uint64_t *ops, uint64_t *states);
/* The same over the words of a stretch of the stream given in engine draws: from *rng_state
 * (a word start; in/out) words are generated until exactly `draws` draws are consumed (an
 * error if the stretch does not end on a word boundary or holds more than max_words words);
 * *words = their count. A sharded sweep's rank decodes the stretch between two word starts
 * found by bchk_stream_sync. */
int bchk_sweep_range(bchk_ctx *ctx, double snr_db, uint64_t *rng_state, uint64_t draws, size_t max_words,
                     uint8_t *tx, uint8_t *res, uint8_t *accepted, uint64_t *ops, uint64_t *states,
                     size_t *words);
/* The reference stream's draw structure for a code of dimension k and length n (host only,
 * no device): a word is k information draws (uniform_int_distribution<unsigned short>(0, 1),
 * src/bchCoder.cpp:236-240, redrawn only for the two largest engine values) and polar-method
 * attempts of four draws until ceil(n/2) pairs are accepted (normal_distribution, :243-250).
 * bchk_stream_skip: the engine state and draws after `words` words from `state` (no samples).
 * bchk_stream_sync: from a word start `state`, a word start in [offset, offset + limit) draws
 * on the stream's own parse that depends only on (state, offset, limit) -- the start where
 * every parse state possible at `offset` has merged, not necessarily the first start at or
 * after `offset` -- found WITHOUT parsing the draws before `offset` (neighbouring ranks make
 * the identical call for a shared boundary, so parts tile the stream; a redrawn information bit before
 * `offset`, or no merge before offset + limit, returns 1 = unresolved): *word_offset (draws
 * from `state`) and *word_state. */
int bchk_stream_skip(int k, int n, uint64_t state, uint64_t words, uint64_t *state_out, uint64_t *draws);
int bchk_stream_sync(int k, int n, uint64_t state, uint64_t offset, uint64_t limit, uint64_t *word_offset,
                     uint64_t *word_state);

/* fun(file, decoder, g, gSize, p, e, maxSTNR) (headers/dataForPlot.h:8,
 * src/dataForPlot.cpp:16-116) on the GPU: identical CSV text, written to csv (cap bytes,
 * NUL-terminated). The stream starts from *rng_state (engine state; NULL or 0 = seed) and
 * *rng_state receives the state after the last word consumed, exactly where the
 * reference's global engine would be. batch = codewords per GPU launch (0 = auto). */
int bchk_sweep(bchk_ctx *ctx, long p, long e, double max_snr, uint64_t *rng_state,
               uint64_t seed, size_t batch, char *csv, size_t cap);

/* On-GPU channel front-end (the encode + AWGN step of src/bchCoder.cpp:120-132,243-250 as a
 * batched kernel): words [word0, word0 + B) of a counter-based stream (Philox4x32-10 keyed
 * by seed; word w depends only on (seed, w)) at Eb/N0 snr_db -- uniform information bits,
 * c(x) = info(x) g(x), y = BPSK(c) + N(0, sd) with sd as src/dataForPlot.cpp:45.
 * Coefficient i of info(x) is bit (i % 128) & 31 of output word (i % 128) >> 5 of counter
 * (w low, w high, 0xFFFFFFFF, 128 (i / 128)): counter word 3 is the BIT OFFSET of the 128-bit
 * block here, where the polar stream (bchk_polar_generate_device) passes the block INDEX; the
 * two streams never share a counter and both are kept as they are. The noise of flat element
 * G = w n + position is element G & 1 of the Box-Muller pair (sqrt(-2 ln u1) cos 2 pi u2, ...
 * sin 2 pi u2) of counter (G / 2 low, G / 2 high, 0x5EED, 0), u = (a 2^21 + (b >> 11) + 1)
 * 2^-53 from output words (a, b) = (0, 1) for u1 and (2, 3) for u2. The same
 * distribution as the reference's words, NOT its minstd_rand0 stream (bchk_generate_host is
 * the bit-exact one). d_tx [B][n] u8, d_y [B][n] f64 on device. */
int bchk_generate_device(bchk_ctx *ctx, double snr_db, size_t B, uint64_t seed, uint64_t word0,
                         uint8_t *d_tx, double *d_y, void *stream);
/* fun() (src/dataForPlot.cpp:16-74) end to end on the GPU: words from bchk_generate_device,
 * decode and counters fused (bchk_decode_count_device), Eb/N0 0..max_snr step 0.5, each point
 * until p words or e frame errors (the e-th error cut exactly in word order). CSV lines as
 * bchk_sweep (statistically the reference's, not byte-identical); seconds = wall time,
 * words = words decoded. One divergence in the BER column: a word the decoder never accepts
 * is compared against the row left at its index in the batch buffer (zero in the first batch,
 * else that row's last accepted word), whereas fun() compares it against the previous word's
 * decision (its `decoded` buffer is shared, src/dataForPlot.cpp:25,52). FER, decodes,
 * comparisons and sums are unaffected only when every word is accepted; unaccepted words are
 * rare (none in the fixtures at n <= 63). bchk_sweep keeps fun()'s carry exactly. */
int bchk_sweep_device(bchk_ctx *ctx, long p, long e, double max_snr, uint64_t seed, size_t batch,
                      char *csv, size_t cap, double *seconds, uint64_t *words);

int bchk_sync(bchk_ctx *ctx);
/* the context's HIP stream (hipStream_t) */
void *bchk_stream(bchk_ctx *ctx);
/* Kernel-time profiling with HIP events recorded on the launch stream around each decode
 * call's three stages: [0] the lane-per-codeword fast kernel (+ the control memset),
 * [1] the exact wave-per-codeword kernel, [2] the workgroup-cooperative kernel for heavy
 * codewords. read() returns the summed milliseconds per stage since the last read and the
 * number of decode calls, then resets. */
int bchk_profile(bchk_ctx *ctx, int enable);
int bchk_profile_read(bchk_ctx *ctx, double *ms3, uint64_t *launches);
/* The same per stage: [0] fast, [1] exact first pass, [2] cooperative, [3] analytic tail
 * kernel (bchk_set_analytic); bchk_profile_read's exact stage is [1] + [3]. */
int bchk_profile_read_stages(bchk_ctx *ctx, double *ms4, uint64_t *launches);
/* Codewords the last decode call handed from the fast path to the exact kernel, and from
 * the exact kernel to the cooperative kernel (synchronises the context's stream). */
int bchk_path_counts(bchk_ctx *ctx, uint64_t *to_exact, uint64_t *to_coop);
/* Codewords the last decode call's exact first pass handed to the analytic tail kernel. */
int bchk_tail_count(bchk_ctx *ctx, uint64_t *to_tail);
/* Outcomes of the last call's analytic tail: [0] handed on to the cooperative kernel,
 * [1] finished from the candidate codewords, [2] split (exact chunks below the earliest
 * candidate within the tightened bound, then the candidates), [3] exact chunks of [2],
 * [4] enumeration steps (64 nodes each) summed, [5] their maximum over codewords. */
int bchk_tail_stats(bchk_ctx *ctx, uint64_t *out6);
/* The last call's cooperative-kernel counters (m >= 7): [0] chunks decoded again densely on
 * the acceptor's request (more candidates than a ring slot keeps; BCHK_LONG_REC=0..2 in the
 * environment at bchk_create sets the records per slot, default 2), [1] heavy codewords the
 * cooperative kernel started. */
int bchk_coop_stats(bchk_ctx *ctx, uint64_t *out2);
/* Diagnostics (context created with BCHK_TAIL_DIAG=1 in the environment): the last call's
 * per-codeword analytic-tail records, 8 u64 each -- codeword, cycles of prep, of the exact
 * chunks, of the plan, enumeration steps, mode | reason << 8 | split chunks << 16, cycles
 * after the plan, decodes. count = records written (may exceed items). */
int bchk_tail_diag_read(bchk_ctx *ctx, uint64_t *out, size_t items, uint64_t *count);
/* Diagnostics of experiment builds (BCHK_AN_PROF, lib/libbchk_anprof.so): per record of
 * bchk_tail_diag_read, 8 u64 of enumeration cycles by step phase -- pops, loads and single
 * children, leaf runs, stack pushes, emission batches, their cycles, leaf-run rounds, steps;
 * the record at index items - 1 of a 32768-record read holds the first pass's cycles summed
 * over its codewords -- prep, decode, acceptance, outputs, chunks, codewords (zeros in the
 * product build). */
int bchk_tail_prof_read(bchk_ctx *ctx, uint64_t *out, size_t items);
/* Enable (default) or disable the fast path; results are identical either way. */
int bchk_set_fast_path(bchk_ctx *ctx, int enable);
/* Enable (default) or disable the analytic tail of the exact kernel (n <= 63, decode
 * variant): a codeword still searching after the chunk limit is finished from its candidate
 * codewords -- those within t of some test pattern whose path metric can still improve
 * (KanekoKernelProcessor.cpp:361-405 replayed over them) -- instead of decoding every test
 * pattern in the cooperative kernel. Results are identical either way. */
int bchk_set_analytic(bchk_ctx *ctx, int enable);
/* 64-pattern chunks the exact kernel decodes before the analytic tail / the hand-off to
 * the cooperative kernel (default 1; 0 = neither: the exact kernel decodes everything). */
int bchk_set_chunk_limit(bchk_ctx *ctx, uint32_t chunks);

/* Enable (default) or disable the syndrome decoding table of the search kernels: for
 * n <= 63 and m (t - 1) <= 30, Decoder::decode of a test pattern is a lookup of its
 * normalised syndrome in a table of the weight <= t coset leaders (csrc/bchk_syndtab.h)
 * instead of Berlekamp-Massey + Chien. Results are identical either way. */
int bchk_set_syndrome_table(bchk_ctx *ctx, int enable);
/* The resident waves of the first exact pass as the next decode call would launch it (the
 * table setting above chooses the kernel). For n <= 63 wave g takes item g of the fast
 * kernel's queue, and the items from `waves` upward are claimed. */
int bchk_first_pass_waves(const bchk_ctx *ctx, uint32_t *waves);
/* Host-side decode through that table (no GPU): for odd syndromes synd[i][0..t) =
 * S_1, S_3, ..., S_{2t-1}, ok[i] = 1 iff Decoder::decode succeeds, and err[i] (may be
 * NULL) = the flipped positions as a bit mask. BCHK_EINVAL when (m, t) has no table.
 * Test/diagnostic entry point. */
int bchk_syndrome_table_query(int m, int t, const uint32_t *synd, size_t N, uint8_t *ok,
                              uint64_t *err);
/* Size of that table: distinct keys, bytes, longest probe sequence (buckets). */
int bchk_syndrome_table_info(int m, int t, uint64_t *keys, uint64_t *bytes, uint32_t *max_probe);

/* Which kernels a context for (m, t) would launch, from the dispatch functions bchk_create
 * itself calls (no device needed): out[0] = TMAX of the instantiated kernel set, out[1] = a
 * fast kernel (n <= 63) or first-pattern kernel (m >= 7) precedes the search kernel,
 * out[2] = the lane pre-pass of the first-pattern kernel, out[3] = the first-pattern
 * kernel's selection variant (calls without a stats record), out[4] = the search kernels
 * decode through the syndrome table, out[5] = the analytic tail kernel; out[6], out[7] = 0.
 * BCHK_EINVAL for every (m, t) bchk_create refuses. */
int bchk_kernel_info(int m, int t, int32_t out[8]);

/* ---- SC-list decoding of polar codes (the reference's vendored library, which its own
 * CMake target does not build: headers/external/MixedKernelListDecoder.h:10-42). Pinned to
 * that library compiled as it stands, for kernels below 64: decode, encode and the kernel
 * LLRs are compared bit for bit with its recorded outputs (tests/golden/polar_ref_*.txt.gz,
 * tests/test_polar_reference.py). LLR sign at this boundary: negative favours bit 1, as the
 * reference's code reads it (MixedKernelListDecoder.cpp:80, :114; its header comment at :36
 * says the opposite and is not what the code does). The 64 x 64 kernel's LLRs have no
 * reference to compare with (TrellisKernelProcessor.cpp:71-72 refuses the size). */
typedef struct bchk_polar bchk_polar;
/* Replaces CMixedKernelListDecoder(std::istream& Spec, unsigned ListSize)
 * (out/external/MixedKernelListDecoder.cpp:9): spec is the text of the reference's code
 * specification (out/external/MixedKernelEncoder.cpp:7-98: "N K d layers #shortened
 * #punctured", kernel names, shortened / punctured symbols, U - K freezing constraints).
 * Kernels: Arikan ("A") layers; the library's named kernels "G" (3 x 3, rows 100 / 110 / 011)
 * and "A5" (5 x 5, rows 10000 / 11000 / 10100 / 10001 / 11110: what CA5Kernel::Multiply
 * computes, TruncatedArikanKernel.cpp:204-216 -- the A5[] array at :251-258 has the last two
 * rows exchanged and is not what the library encodes or decodes with), names in any case as
 * Kernel.cpp:234-274 compares them, decoded by the library's own recursive f/g processors
 * (TruncatedArikanKernel.cpp:152-184, :341-397), whose per-path state (one float per element
 * for G; three floats and a bit for A5) is carried with the path through clones and
 * suspended launches. The reference itself copies G's state on a clone only at phase 0 of
 * the whole code (:141-149, KernelListEngine.cpp:361), so with list_size > 1 its output is
 * defined only where every G is the innermost layer; there, and at list_size 1, and for A5
 * anywhere, the lists are the reference's bit for bit, and elsewhere they are those of the
 * state travelling with the path. And matrix kernels ("-file" / "<file", a size and size^2
 * entries, Kernel.cpp:93-107 -- e.g. BCH-derived kernels) of size <= 64, whose kernel LLRs are
 * the trellis min-sum of out/external/TrellisKernelProcessor.cpp:234-294 (polar_mixed.hip):
 * coset enumeration below 16, the trellis for 16..32 (at most 2^12 states per depth), and an
 * exact ordered-statistics search above 32 (the 64 x 64 extended-BCH kernel; the reference's
 * trellis processor stops below 64) -- the same value bit for bit;
 * 1 <= list_size <= 32, lengths whose per-wave state fits the 160 KiB LDS (for all-Arikan
 * codes about 4.4 bytes per symbol and path: U <= 2048 at L = 16, 4096 at L = 8, 8192 at
 * L = 4; longer ones decode with bchk_polar_create_tiered). Kernel files are read relative to
 * kdir. */
int bchk_polar_create(const char *spec, int list_size, int device, bchk_polar **out);
int bchk_polar_create_kdir(const char *spec, const char *kdir, int list_size, int device, bchk_polar **out);
/* The same decoder for all-Arikan codes up to U = 16384 at any list size: the LLR layers S_l
 * and partial sums C_l of the layers l <= split (and the codeword C_0) live in a workspace in
 * device memory, shared between the paths of a list and copied only when written (Tal and
 * Vardy's lazy copy); the layers below the split stay in LDS. Lists are bit for bit those of
 * bchk_polar_create_kdir. split = -1: the library chooses -- the smallest split whose LDS part
 * fits 160 KiB, then further layers out while that lets one more wave onto a CU, up to 8; split in
 * 1..layers: the boundary exactly there. BCHK_EINVAL before any device call for a matrix or named
 * layer, a split out of range, U > 16384, or an LDS part above 160 KiB at the split asked for.
 * The workspace (grid x bytes per workgroup) is allocated here and freed by bchk_polar_destroy;
 * the grid shrinks to keep it within BCHK_POLAR_WORKSPACE_MB MiB (default 1024). Every other
 * bchk_polar_* call takes such a context; the genie-aided SC calls keep their own LDS limit. */
int bchk_polar_create_tiered(const char *spec, const char *kdir, int list_size, int device, int split,
                             bchk_polar **out);
/* The tiered state for codes with matrix or named layers (and, through the same kernel,
 * all-Arikan ones): polar_mixed_tiered.hip. For every layer j < split (layers counted from the
 * channel side, 1 <= split <= layers) the layer's LLRs S_{j+1}, partial sums C_{j+1}, offset
 * state and a named layer's carried floats live in a per-workgroup workspace in device memory,
 * shared between the paths of a list and copied only when written; the codeword C_0 and the
 * mapped channel LLRs lie there too; the inner layers stay in LDS. Lists are bit for bit those
 * of bchk_polar_create_kdir. split = -1: the rule of bchk_polar_create_tiered applied to this
 * layout. BCHK_EINVAL before any device call for a split out of range, an LDS part above
 * 160 KiB at the split asked for, or a code with an ordered-statistics layer (a matrix kernel
 * above 32, or BCHK_POLAR_ML lowered), which stays on the LDS state. Workspace, grid bound
 * (BCHK_POLAR_WORKSPACE_MB) and the other bchk_polar_* calls as for bchk_polar_create_tiered. */
int bchk_polar_create_tiered_mixed(const char *spec, const char *kdir, int list_size, int device, int split,
                                   bchk_polar **out);
/* Where a context keeps its list state (any may be NULL): the split in use (0: all in LDS), LDS
 * bytes per workgroup, workspace bytes per workgroup (0 unless tiered), workgroups of a launch. */
int bchk_polar_state_info(const bchk_polar *pc, int *split, uint64_t *lds_bytes, uint64_t *workspace_bytes, int *grid);
void bchk_polar_destroy(bchk_polar *pc);
/* N (transmitted length), K, U (unshortened length), L */
int bchk_polar_params(const bchk_polar *pc, int *n, int *k, int *unshortened, int *list_size);
/* Replaces Decode(pLLR, pInfVectorList, pCodewordList) (MixedKernelListDecoder.cpp:211-268),
 * batched: llr [B][N] float, log P(0)/P(1) as the decoder reads them (bit 1 when < 0);
 * per codeword the list, best path first: info [B][L][K], cw [B][L][N] (may be NULL),
 * metric [B][L] (path metrics, 0 = the hard decision), count [B] (rows written; rows past
 * it are left as they were). A code of dimension K = 0 is decoded like any other: count 1, the
 * frozen word and its metric, no information byte written (info must still be non-NULL); only
 * the entry points that need Eb/N0, and with it the rate -- bchk_polar_generate_device,
 * bchk_polar_sweep_device, bchk_polar_genie_run, bchk_polar_design_genie -- refuse it. */
int bchk_polar_decode_host(bchk_polar *pc, const float *llr, size_t B, uint8_t *info,
                           uint8_t *cw, float *metric, int32_t *count);
int bchk_polar_decode_device(bchk_polar *pc, const float *d_llr, size_t B, uint8_t *d_info,
                             uint8_t *d_cw, float *d_metric, int32_t *d_count, void *stream);
/* Codes with a search layer (a matrix kernel above 32, e.g. the 64 x 64 extended-BCH kernel):
 * one codeword's list decode can take seconds, so a decode call is a series of kernel launches
 * of about 50 ms each (environment BCHK_POLAR_BUDGET_MS; 0 = one launch per call): a codeword
 * is suspended between two search items and resumed by the next launch, with identical
 * results. A budgeted decode call is synchronous on the stream it is given: it waits for
 * that stream after every launch and returns when the batch is decoded (bchk_polar_decode_device
 * too, on the caller's stream). One context must not be used from two streams (or threads) at
 * once: the per-codeword states, the save slots of suspended codewords and the launch counters
 * belong to the context. Every launch makes progress whatever the budget (a wave always works on
 * the first unfinished codeword it meets, and a search runs at least one round per launch); a
 * launch that leaves codewords unfinished and reports none is an error (BCHK_EHIP), not a hang.
 * The launches the last call took (1 for codes without a search layer or with the budget off). */
int bchk_polar_last_launches(const bchk_polar *pc, uint64_t *launches);
/* Device scratch the context holds for budgeted calls, in bytes: 4 per codeword of the largest
 * batch so far, one save slot of *save_stride bytes (may be NULL; 0 for codes without a search
 * layer) per workgroup of the largest grid so far, and two counter words; plus a tiered
 * context's workspace. */
int bchk_polar_scratch_bytes(const bchk_polar *pc, uint64_t *bytes, uint64_t *save_stride);
/* CMixedKernelEncoder::Encode (MixedKernelEncoder.cpp:142-177), host side: info [B][K] ->
 * codewords [B][N]. */
int bchk_polar_encode_host(const bchk_polar *pc, const uint8_t *info, size_t B, uint8_t *cw);
int bchk_polar_sync(bchk_polar *pc);
void *bchk_polar_stream(bchk_polar *pc);

/* ---- Polar FER simulation on the device: the BPSK part of the vendored simulator's
 * iteration (out/external/Simulator.cpp:104-114, :139-335, headers/external/Modem.h:64-78) as
 * kernels (csrc/polar_channel.hip), over AWGN and, through the *_channel* entry points, real
 * Rayleigh fading with ideal channel knowledge and the BSC (Simulator.cpp:179-191). Device pointers; each call enqueues on `stream` (NULL =
 * the context's stream); B = 0 is a no-op; B > 2^32 - 1 is BCHK_EINVAL. */
/* CMixedKernelEncoder::Encode (MixedKernelEncoder.cpp:142-177) as a kernel, bit for bit
 * bchk_polar_encode_host for every code bchk_polar_create accepts: d_info [B][K] -> d_cw [B][N]. */
int bchk_polar_encode_device(bchk_polar *pc, const uint8_t *d_info, size_t B, uint8_t *d_cw, void *stream);
/* Words [word0, word0 + B) of a counter-based stream (Philox4x32-10 keyed by seed, the
 * generator of bchk_generate_device; word w depends only on (seed, w)) at Eb/N0 snr_db:
 * uniform information bits (counter (w low, w high, 0xFFFFFFFF, index of the 128-bit block)),
 * the codeword, BPSK with bit 1 -> +1 (Modem.h:64), y = x + sigma z in double with sigma =
 * sqrt(0.5 10^(-snr_db/10) N / K) (Simulator.cpp:108, N the transmitted length; z for flat
 * element G = w N + position is one of the Box-Muller pair of counter (G / 2, tag 0x5EED)),
 * LLR = (float)(-2 y / sigma^2) (Modem.h:78; positive favours 0). d_info [B][K] and d_cw
 * [B][N] may each be NULL; d_llr [B][N] float. Statistically the simulator's stream, NOT its
 * GSL mt19937 stream bit for bit (the same caveat as bchk_generate_device). */
int bchk_polar_generate_device(bchk_polar *pc, double snr_db, size_t B, uint64_t seed, uint64_t word0,
                               uint8_t *d_info, uint8_t *d_cw, float *d_llr, void *stream);
/* The channels of the simulator's loop (Simulator.cpp:179-191). The entry points without a
 * channel argument mean BCHK_CHANNEL_AWGN. */
#define BCHK_CHANNEL_AWGN 0     /* y = x + sigma z; param = Eb/N0 in dB                          */
#define BCHK_CHANNEL_RAYLEIGH 1 /* y = h x + sigma z, h known to the receiver; param = the       */
                                /* average Eb/N0 in dB                                           */
#define BCHK_CHANNEL_BSC 2      /* y = +-x; param = the crossover probability p, 0 < p <= 0.5    */
/* bchk_polar_generate_device over any of the three channels. The stream is the same: for a given
 * (seed, word0) d_info and d_cw are byte for byte those of bchk_polar_generate_device whatever
 * the channel, x is BPSK with bit 1 -> +1 (Modem.h:64) and z the Gaussian of flat element
 * G = w N + position. The Rayleigh channel and the BSC draw one more uniform per element:
 *   u(G) = (a 2^21 + (b >> 11) + 1) 2^-53 in (0, 1], (a, b) = output words (0, 1) when G is even
 *   and (2, 3) when G is odd of the Philox4x32-10 call with counter (G / 2 low, G / 2 high,
 *   0xFAD1, 0) under the key (seed low, seed high).
 * BCHK_CHANNEL_AWGN: bchk_polar_generate_device bit for bit.
 * BCHK_CHANNEL_RAYLEIGH (Simulator.cpp:183-187, SimpleChannels.h:139): h = sqrt(-log u), the
 *   gsl_ran_rayleigh draw of scale 1 / sqrt 2, so E[h^2] = 1; y = h x + sigma z in double, sigma
 *   as for AWGN at the same Eb/N0 (Simulator.cpp:108: with E[h^2] = 1 the average Eb/N0);
 *   LLR = (float)(-2 h y / sigma^2), evaluated as ((-2 h) y) / sigma^2 (Modem.h:78 with the
 *   fading factor).
 * BCHK_CHANNEL_BSC (Simulator.cpp:188-191, :114): y = x where u > p, -x where u <= p;
 *   LLR = (float)(-2 y) = +-2, the reference's noise variance 1 -- not log((1 - p) / p): the
 *   decoder is min-sum, its decisions do not depend on the scale. Counter [6] of
 *   bchk_polar_count_device then counts the flips.
 * d_h [B][N] and d_y [B][N], doubles, may each be NULL and are written only when given: the
 * fading factor h (Rayleigh only) and the channel output y ahead of the demodulator. One
 * launch, as before. BCHK_EINVAL before any device call, the message naming the argument: an
 * unknown channel; p outside (0, 0.5] or NaN; d_h given for AWGN or the BSC; K = 0 (as
 * bchk_polar_generate_device: the code has no rate). The BEC (commented out at
 * Simulator.cpp:193) and higher-order modems are not built; block, correlated and Rician fading
 * are the *_fading* entry points below. */
int bchk_polar_generate_channel_device(bchk_polar *pc, int channel, double param, size_t B, uint64_t seed,
                                       uint64_t word0, uint8_t *d_info, uint8_t *d_cw, float *d_llr, double *d_h,
                                       double *d_y, void *stream);
/* The counters of CSimulator::Iterate (Simulator.cpp:201-318) for one decoded batch -- sent
 * d_info_tx [B][K], d_cw_tx [B][N], the channel's d_llr [B][N], and bchk_polar_decode_device's
 * d_info [B][L][K], d_cw [B][L][N] (required: the counters need the codeword rows), d_count
 * [B] -- added into the device array d_out8 (uint64_t[8]):
 *   [0] words
 *   [1] block errors: row 0's information bits differ from the sent ones, or count <= 0 (:233-255)
 *   [2] information bit errors of row 0, over block-error words (:245-249, :283)
 *   [3] code bit errors of row 0, over block-error words (:250-254, :284)
 *   [4] ML errors: block error, count > 0 and CurCorr >= MLCorr, the double sums of +-llr[i]
 *       over i = 0..N-1 in index order (:264-287)
 *   [5] list errors: block error and the sent codeword is not among rows 1..count-1 (:263, :288-318)
 *   [6] raw bit errors: positions where (sent bit ? -llr : llr) < 0 (:203-208)
 *   [7] words with count <= 0
 * A word with count <= 0 adds to [0], [1], [5], [6] and [7] only: the reference would compare
 * the stale buffers of the previous word there. d_flags ([B] bytes, may be NULL) receives per
 * word bit 0 = block error, bit 1 = ML error, bit 2 = list error. */
int bchk_polar_count_device(bchk_polar *pc, const uint8_t *d_info_tx, const uint8_t *d_cw_tx, const float *d_llr,
                            const uint8_t *d_info, const uint8_t *d_cw, const int32_t *d_count, size_t B,
                            uint64_t *d_out8, uint8_t *d_flags, void *stream);
/* One Eb/N0 point of bchk_polar_sweep_device: the counters of bchk_polar_count_device. */
typedef struct bchk_polar_point {
    double snr_db;
    uint64_t c[8];
} bchk_polar_point;
/* The simulation loop end to end on the device: `points` points at snr_from + i snr_step into
 * the host array out; each generates (bchk_polar_generate_device, stream `seed`), decodes and
 * counts batches of at most `batch` words (0 = sized from the context's grid) until max_words
 * words or max_errors block errors. A point is cut exactly in word order: its counters cover
 * the words up to and including the one that carries the max_errors-th block error, and the
 * word index runs on across points (the next point starts at the word after the cut), so the
 * records are a function of the arguments other than `batch`. Synchronous, on the context's
 * stream, with buffers the context owns; seconds (may be NULL) = wall time, words_decoded (may
 * be NULL) = words sent through the decoder (whole batches, the cut ones included). */
int bchk_polar_sweep_device(bchk_polar *pc, double snr_from, double snr_step, int points, uint64_t max_words,
                            uint64_t max_errors, uint64_t seed, size_t batch, bchk_polar_point *out,
                            double *seconds, uint64_t *words_decoded);
/* The same loop over `channel` (bchk_polar_generate_channel_device): the points are Eb/N0 values
 * in dB for AWGN and Rayleigh and crossover probabilities p for the BSC (the record's snr_db
 * field then holds p), from + i step. The same exact cut in word order, the word index running
 * on across points. Every point's parameter is checked before any work (BCHK_EINVAL for an
 * unknown channel or a p outside (0, 0.5]); BCHK_CHANNEL_AWGN gives bchk_polar_sweep_device's
 * records exactly. */
int bchk_polar_sweep_channel_device(bchk_polar *pc, int channel, double from, double step, int points,
                                    uint64_t max_words, uint64_t max_errors, uint64_t seed, size_t batch,
                                    bchk_polar_point *out, double *seconds, uint64_t *words_decoded);

/* ---- The fading models with a parameter (headers/external/Simulation/RayleighBlockChannel.h,
 * RayleighCorrelatedChannel.h, RacianChannel.h). Common to the three: the stream of
 * bchk_polar_generate_channel_device (d_info, d_cw and the Gaussian z of an element are those of
 * every other channel), y = h x + sigma z in double with sigma from the average Eb/N0 snr_db as
 * for BCHK_CHANNEL_RAYLEIGH (every model has E[h^2] = 1), LLR = (float)(((-2 h) y) / sigma^2),
 * the receiver knowing h. Word w depends only on (seed, w, kind, param, snr_db). */
#define BCHK_FADING_BLOCK 0      /* param = the block size S, an integer >= 1: positions [b S,      */
                                 /* (b + 1) S) of a word share the factor BCHK_CHANNEL_RAYLEIGH     */
                                 /* gives the block's first element (h = sqrt(-log u(w N + b S))),  */
                                 /* the last block may be short; S = 1 is BCHK_CHANNEL_RAYLEIGH bit */
                                 /* for bit, S >= N one factor per word                             */
#define BCHK_FADING_CORRELATED 1 /* param = rho, 0 <= rho < 1: elements 2 q and 2 q + 1 of a word   */
                                 /* (QAM symbol q; the last is half filled when N is odd) share     */
                                 /* h_q = sqrt((a_q^2 + b_q^2) / 2), a and b two unit-variance      */
                                 /* Gaussian sequences of covariance rho^|i - j|, fresh per word:   */
                                 /* g_0 = z_0, g_q = fma(rho, g_{q-1}, c z_q), c = sqrt(1 - rho^2)  */
                                 /* in double, the product rounded before the fma; (z_q of a, z_q   */
                                 /* of b) = the Box-Muller pair of counter (w low, w high, 0xC022, q) */
#define BCHK_FADING_RICIAN 2     /* param = the K-factor, finite and >= 0: h = sqrt((v + s z1)^2 +  */
                                 /* (s z2)^2), v = sqrt(K / (K + 1)), s = sqrt(1 / (2 (K + 1))),    */
                                 /* (z1, z2) = the Box-Muller pair of counter (w low, w high,       */
                                 /* 0x21CE, position); K = 0 is Rayleigh fading in law              */
/* bchk_polar_generate_channel_device, _sweep_channel_device and _sweep_q8_device over a fading
 * model: (kind, param) choose it, snr_db / the points are average Eb/N0 values in dB. d_h
 * receives the factors of every kind. BCHK_EINVAL before the context is touched, the message
 * naming the argument: a kind outside 0..2; a block size below 1 or no integer; rho outside
 * [0, 1) or NaN; a K-factor negative, NaN or infinite. Everything else as the calls named. */
int bchk_polar_generate_fading_device(bchk_polar *pc, int kind, double param, double snr_db, size_t B,
                                      uint64_t seed, uint64_t word0, uint8_t *d_info, uint8_t *d_cw, float *d_llr,
                                      double *d_h, double *d_y, void *stream);
int bchk_polar_sweep_fading_device(bchk_polar *pc, int kind, double param, double snr_from, double snr_step,
                                   int points, uint64_t max_words, uint64_t max_errors, uint64_t seed, size_t batch,
                                   bchk_polar_point *out, double *seconds, uint64_t *words_decoded);

/* ---- Fixed-point SC-list decoding: int8 LLRs (csrc/polar_sclist_q8.hip). The
 * vendored library's USE_INT8 configuration (SeqConfigOrig.h:186-194, SoftProcessing.cpp:643-1146)
 * with symmetric saturation, for all-Arikan codes with every path's state in LDS. The contract:
 *   sign       LLRs are int8_t, negative favours bit 1 (as everywhere at this boundary)
 *   load       a value of -128 is read as -127; a punctured symbol loads 0, a shortened one +127
 *   f step     f(a, b) = sgn(a) sgn(b) min(|a|, |b|), 0 if either operand is 0
 *   g step     g(a, b, u) = clamp(u ? b - a : b + a, -127, +127)
 *   decisions  the hard decision is v < 0; a decision against it costs |v|: R <- R - |v|
 *   list       candidate order, kills, clones, free-index stack and final order are exactly those
 *              of the f32 decoder (the same device routines)
 *   metrics    written to the float metric buffer as exact integers (|R| <= 127 U < 2^24)
 * So wherever no g step saturates, the lists are bit for bit those of bchk_polar_decode_* on the
 * same values as floats. (The library's AVX path saturates at -128, where its abs wraps, and it
 * loads 0x3F for a shortened symbol, MixedKernelEncoder.cpp:195; neither is followed.)
 * Per path and symbol the state takes about 1.4 bytes instead of 4.4: (2048, 1024) at L = 32 and
 * (4096, 2048) at L = 16 fit the 160 KiB. BCHK_EINVAL before any device call, with a message
 * naming it, for a code with a matrix or named layer, and for a length whose int8 state exceeds
 * 160 KiB. The context takes every other bchk_polar_* call (encode, generate, count, genie,
 * state_info) but decodes only through the two calls below, which in turn refuse (BCHK_EINVAL)
 * a context of any other bchk_polar_create*; bchk_polar_decode_* and bchk_polar_sweep_*device
 * refuse this one. */
int bchk_polar_create_q8(const char *spec, const char *kdir, int list_size, int device, bchk_polar **out);
/* The int8 decoder past the LDS budget (csrc/polar_sclist_q8_tiered.hip): the
 * contract above in the tiered state of bchk_polar_create_tiered. The layers 1..split of every
 * path lie in a per-workgroup device-memory workspace, the LLRs as bytes (about 1.4 U L bytes per
 * workgroup where the f32 tiered state takes 4.4 U L), so every all-Arikan code up to U = 16384
 * decodes at every list size up to 32, and where bchk_polar_create_q8 also takes the code the
 * lists are its lists bit for bit. split = -1: the rule of bchk_polar_create_tiered applied to
 * this state's LDS bytes; 1..layers is taken as given. BCHK_EINVAL before any device call, with a
 * message, for a matrix or named layer (named as above), a split outside -1 and 1..layers,
 * U > 16384, a list size outside 1..32, and an LDS part above 160 KiB at the split asked for.
 * Workspace, its bound (BCHK_POLAR_WORKSPACE_MB), bchk_polar_state_info and
 * bchk_polar_scratch_bytes as for bchk_polar_create_tiered; the context is an int8 context in
 * every call: it decodes and sweeps through the bchk_polar_*_q8_* calls below only. */
int bchk_polar_create_q8_tiered(const char *spec, const char *kdir, int list_size, int device, int split,
                                bchk_polar **out);
/* llr [B][N] int8_t; info, cw, metric, count as bchk_polar_decode_host / _device. */
int bchk_polar_decode_q8_host(bchk_polar *pc, const int8_t *llr, size_t B, uint8_t *info, uint8_t *cw,
                              float *metric, int32_t *count);
int bchk_polar_decode_q8_device(bchk_polar *pc, const int8_t *d_llr, size_t B, uint8_t *d_info, uint8_t *d_cw,
                                float *d_metric, int32_t *d_count, void *stream);
/* The demodulator's discretisation (NORMALIZE_MODEM, Modem.h:71-76) as one element-wise kernel on
 * `stream` (NULL = the context's; any context): d_q[i] = clamp(rint(d_llr[i] * scale), -qmax,
 * qmax) for i < count, the product formed in f32, ties to even, NaN -> 0, +-inf -> +-qmax.
 * 1 <= qmax <= 127 (63 is the library's MTYPE_UPPER_BOUND for int8) and a positive finite scale,
 * else BCHK_EINVAL; count = 0 is a no-op. */
int bchk_polar_quantize_device(bchk_polar *pc, const float *d_llr, size_t count, float scale, int qmax, int8_t *d_q,
                               void *stream);
/* bchk_polar_sweep_channel_device on an int8 context: the same loop, stream, exact cut and
 * channels, each batch going generate -> quantize (scale, qmax) -> int8 decode -> count (the
 * counters read the channel's f32 LLRs). scale and qmax are checked as by
 * bchk_polar_quantize_device before any work. */
int bchk_polar_sweep_q8_device(bchk_polar *pc, int channel, double from, double step, int points,
                               uint64_t max_words, uint64_t max_errors, uint64_t seed, size_t batch,
                               bchk_polar_point *out, double *seconds, uint64_t *words_decoded, float scale,
                               int qmax);
/* The same on a fading model (bchk_polar_sweep_fading_device). */
int bchk_polar_sweep_q8_fading_device(bchk_polar *pc, int kind, double param, double snr_from, double snr_step,
                                      int points, uint64_t max_words, uint64_t max_errors, uint64_t seed,
                                      size_t batch, bchk_polar_point *out, double *seconds, uint64_t *words_decoded,
                                      float scale, int qmax);

/* ---- BCH polar-kernel construction and the column-permutation search (root bchCoder.cpp;
 * csrc/kernel_search.hip). Kernels are row-major l x l bytes (0/1). */
/* makeMatrix (root bchCoder.cpp:356-389): the nested extended-BCH kernel of size 2^power
 * (2 <= power <= 6), GF(2^power) from the reference's primitive polynomials
 * (src/main.cpp:14-15). Columns in power order: column 0 the extension, column p + 1 the
 * position of alpha^p. */
int bchk_kernel_ebch(int power, uint8_t *K);
/* swapColumns' reordering (root bchCoder.cpp:478-496): columns 0..2 kept, column i >= 3
 * takes the column of the field element i. */
int bchk_kernel_field_order(int power, const uint8_t *K, uint8_t *out);
/* The operation counts (SumCount, CmpCount; headers/external/misc.h:84-93) a
 * CTrellisKernelProcessor (out/external/TrellisKernelProcessor.cpp:69-294) spends on
 * GetLLRs(1, phase, zero known inputs, llr) for every phase 0..l-1 of the invertible kernel
 * K (2 <= l <= 32), the score the column search minimises (root bchCoder.cpp:505-515). */
int bchk_kernel_trellis_cost(const uint8_t *K, int l, const float *llr, int device, uint64_t *sum,
                             uint64_t *cmp);
/* The same score for every column map j -> B j with B = L.U (randomInvertibleMatrix, root
 * bchCoder.cpp:766-785) of a 2^power kernel: sum / cmp hold 2^(power (power - 1)) entries,
 * indexed by the candidate code whose bit d is the d-th bit randomInvertibleMatrix draws
 * (row i: l[i][0..i-1], then u[i][i+1..power-1]). */
int bchk_kernel_column_costs(int power, const uint8_t *K, const float *llr, int device, uint64_t *sum,
                             uint64_t *cmp);
#define BCHK_KSEARCH_EXHAUSTIVE 0 /* every L.U product, in code order                    */
#define BCHK_KSEARCH_RANDOM 1     /* randomSwapColumns: `count` random L.U products drawn  */
                                  /* from the reference's engine (state *rng_state, in/out) */
/* randomSwapColumns (root bchCoder.cpp:541-699): the candidate accepted last under the
 * reference's rule (both counts strictly below the best so far, :651-657), its permuted
 * kernel best[k][j] = K[k][perm[j]] (:627-629; best / perm may be NULL), its counts and its
 * index in the candidate sequence (-1: none). Scores come from the GPU (one launch over all
 * candidates), the acceptance is replayed on the host in candidate order. */
int bchk_kernel_column_search(int power, const uint8_t *K, const float *llr, int mode, uint64_t count,
                              uint64_t *rng_state, int device, uint8_t *best, uint32_t *perm,
                              uint64_t *best_sum, uint64_t *best_cmp, int64_t *best_index);

/* ---- BEC polarisation behaviour of a kernel and the code design built on it
 * (csrc/kernel_bec.hip, csrc/polar_design.cpp). The decoder's conventions: c = sum_i u_i row_i,
 * phase i is decoded knowing u_0..u_{i-1}. With the columns of E erased and S kept, phase i is
 * uncorrectable iff row_i|S lies in the span of {row_j|S : j > i}. K must be invertible
 * (BCHK_EINVAL otherwise, as for a kernel file). */
/* The primitive: per erasure pattern (bit j = column j erased; bits >= l ignored) the mask of
 * uncorrectable phases (bit i = phase i). 2 <= l <= 64. */
int bchk_kernel_bec_masks(const uint8_t *K, int l, const uint64_t *patterns, size_t n, int device,
                          uint64_t *masks);
/* Exact polarisation behaviour, 2 <= l <= 32: counts[i * (l + 1) + w] = the erasure patterns
 * of weight w that leave phase i uncorrectable, all C(l, w) of them enumerated for every
 * 0 <= w_lo <= w <= w_hi <= l (other weights are left 0). This is the table of the
 * reference's CBECCapacityEvaluator (out/external/CapacityEvaluator.cpp:100-140). The
 * enumeration is cut into kernel launches of at most 2^28 patterns. */
int bchk_kernel_bec_behaviour(const uint8_t *K, int l, int w_lo, int w_hi, int device, uint64_t *counts);
/* The same for any 2 <= l <= 64 with at most `samples` (1..2^40) patterns per weight: a weight
 * with C(l, w) <= samples is enumerated (exact[w] = 1, tried[w] = C(l, w)); any other takes
 * `samples` uniform w-subsets (exact[w] = 0, tried[w] = samples), sample s of weight w being
 * the subset of colex rank r, r uniform below C(l, w) from the Philox4x32-10 stream keyed by
 * seed at counters (s low, s high, w, 0xBEC00000 + attempt) -- a function of (seed, w, s)
 * only, so the result does not depend on how the work is cut into lanes and launches
 * (BCHK_BEC_RUN in the environment = patterns per lane, 1..4095; default sized from the
 * launch). unc[i * (l + 1) + w] = uncorrectable patterns among the tried ones; the estimate
 * of counts is unc C(l, w) / tried. patterns (may be NULL) receives the tried[pattern_weight]
 * patterns of weight pattern_weight, in rank / sample order (room for min(C(l, w), samples)). */
int bchk_kernel_bec_sample(const uint8_t *K, int l, uint64_t samples, uint64_t seed, int device, uint64_t *unc,
                           uint64_t *tried, uint8_t *exact, int pattern_weight, uint64_t *patterns);
/* CBECCapacityEvaluator::GetSubchannelCapacity (CapacityEvaluator.cpp:124-140) restated and
 * pinned to the compiled evaluator (tests/golden/polar_ref_capacity_*.txt.gz: equal bits on
 * every recorded row with C > 0): the capacity of phase `phase` over a BEC of capacity C,
 * 1 - sum_w counts[phase][w] P^w C^(l - w) with P = 1 - C, by the same Horner rule in
 * S = P / C in double. Host only.
 * Divergence: at C = 0 the reference divides by zero and returns NaN; this returns the
 * polynomial's value 1 - counts[phase][l].
 * Domain: the rule is accurate to a few 2^-53 ABSOLUTE, so only while the capacity it returns is
 * well above 1e-16, in practice for C near 1/2. For small C the result is rounding noise of
 * either sign (l = 4, C = 1e-5: -2.2e-16 for a true 1e-20), then -inf or NaN once S^l overflows
 * or pow(C, l) underflows (l = 16: NaN from C = 1e-40; l = 32: -inf at 1e-10) -- reproduced here
 * bit for bit. bchk_polar_design_bec does not use it for matrix layers. */
int bchk_kernel_bec_capacity(const uint64_t *counts, int l, int phase, double C, double *out);
/* A kernel file in the reference's format (Kernel.cpp:93-134): the size, the matrix and, when
 * counts is given, the BEC section CBECCapacityEvaluator's constructor parses -- channel id 3
 * (ec_BEC, headers/external/Simulator.h:13-17) and l rows "0 counts[i][1] .. counts[i][l]".
 * bchk_polar_create_kdir reads such files (it ignores what follows the matrix). Host only. */
int bchk_kernel_write_file(const char *path, const uint8_t *K, int l, const uint64_t *counts);
/* BEC design of a polar code over mixed kernels: `layers` is the specification's kernel-name
 * line ("-e16.txt A A"; files relative to kdir), K the dimension, capacity the design BEC
 * capacity. A matrix layer's table is the BEC section of its file when there is one;
 * otherwise it is computed on the GPU (bchk_kernel_bec_behaviour up to size 32,
 * bchk_kernel_bec_sample with (samples, seed) above), so all-Arikan designs and files with
 * tables need no device. Symbol i has mixed-radix digits (a_0 .. a_{n-1}), a_0 most
 * significant; layer 0 faces the channel (MixedKernelEncoder.cpp:161-173), so its capacity is
 * T_{n-1,a_{n-1}}( .. T_{1,a_1}(T_{0,a_0}(capacity))), T of an "A" layer being C^2 and
 * 2C - C^2 (Kernel.cpp:70-75), and of a matrix layer sum_w (C(l, w) - counts[a][w]) P^w C^(l-w),
 * the sum over correctable patterns: the same polynomial as bchk_kernel_bec_capacity's, but
 * with no negative term, so that it keeps its relative accuracy ((5 l + 4) 2^-53) for the
 * capacities far below 1e-16 that inner layers see (a sampled table's difference is clamped
 * at 0); every capacity is finite and in [0, 1]. The K largest capacities carry information, ties going to
 * the higher index. cap (may be NULL) receives the U capacities; spec receives the text
 * (a named kernel "G" / "A5" in `layers` is BCHK_EINVAL with a message naming it: the
 * library's tables for them are program text, and ML polarisation of the matrix is not what
 * A5's f/g processor achieves; bchk_polar_design_genie takes them)
 * "U K 0 n 0 0", the layer line and "1 f" per frozen symbol, ascending (no shortening,
 * puncturing or dynamic freezing). *needed = the bytes the text takes with its terminator
 * (0 when the arguments were rejected before it was formed); a buffer shorter than that is
 * BCHK_EINVAL. */
int bchk_polar_design_bec(const char *layers, const char *kdir, int K, double capacity, uint64_t samples,
                          uint64_t seed, int device, double *cap, char *spec, size_t spec_len, size_t *needed);

/* ---- Genie-aided SC and the Monte-Carlo AWGN design built on it (csrc/polar_genie.hip,
 * csrc/polar_host.cpp, csrc/polar_design.cpp). Symbol phi of a word is decoded by one SC path
 * with the TRUE u_0..u_{phi-1} (the encoder's inputs, rebuilt from the sent information bits as
 * bchk_polar_generate_device's encoder forms them) fed back: LLR_phi is, bit for bit, the value
 * bchk_polar_decode_device computes for a path whose earlier decisions were u_0..u_{phi-1}
 * (LoadLLRs with 100000 at shortened and 0 at punctured symbols, f/g on Arikan layers, the
 * named kernels' processors on "G" / "A5" layers, coset
 * enumeration or the trellis on matrix layers under the context's per-layer choice,
 * BCHK_POLAR_TRELLIS). Per symbol phi = 0..U-1, frozen symbols included, and per word:
 *   err[phi]  += 1 when (LLR_phi < 0 ? 1 : 0) != u_phi            (the decoder's decision rule)
 *   soft[phi] += q, q = (int64) of c * 65536.0f rounded to nearest even, c = s clamped to
 *                [-32768, 32768], s = u_phi ? -LLR_phi : LLR_phi   (the product is exact in float)
 * The sums are integers: they do not depend on the grid, on how a range of words is split into
 * calls or batches, or on the order of waves. A code with a search layer (a matrix kernel above
 * 32, or BCHK_POLAR_ML on any layer) is BCHK_EINVAL; so is a length whose one-path state exceeds
 * the 160 KiB LDS. Works for any list_size of the context. */
/* One batch: d_info_tx [B][K] sent information bits, d_llr [B][N] channel LLRs; d_err and d_soft
 * ([U] each, device) are ADDED into; d_dec_llr [B][U] float (the decision LLRs) and d_u [B][U]
 * bytes (the rebuilt encoder inputs) may each be NULL -- the rows then go to scratch the context
 * owns, grown (a device allocation) when a call needs more than any before it. Enqueues on
 * `stream` (NULL = the context's stream); B = 0 is a no-op; B > 2^32 - 1 is BCHK_EINVAL. */
int bchk_polar_genie_device(bchk_polar *pc, const uint8_t *d_info_tx, const float *d_llr, size_t B,
                            uint64_t *d_err, int64_t *d_soft, float *d_dec_llr, uint8_t *d_u, void *stream);
/* Words [word0, word0 + words) of bchk_polar_generate_device's stream `seed` at snr_db, in batches
 * of at most `batch` words (0 = sized from the kernel's grid), into buffers the context owns:
 * err and soft (host, [U] each) are overwritten with the sums, a function of (code, snr_db, seed,
 * word0, words) only. Synchronous, on the context's stream. 1 <= words <= 2^31 (BCHK_EINVAL
 * otherwise: |q| <= 2^31, so soft stays inside 64 bits); seconds (may be NULL) = wall time. */
int bchk_polar_genie_run(bchk_polar *pc, double snr_db, uint64_t words, uint64_t seed, uint64_t word0,
                         size_t batch, uint64_t *err, int64_t *soft, double *seconds);
/* Monte-Carlo AWGN design over the kernels of `layers` (as bchk_polar_design_bec): the code
 * "U K 0 n 0 0" with the lowest U - K indices frozen (the rate K / U fixes the noise deviation;
 * the statistics do not depend on the frozen set) goes through bchk_polar_genie_run(snr_db,
 * words, seed, word0 = 0, batch = 0) on `device`; symbol i is better than j when err_i < err_j,
 * on a tie when soft_i > soft_j, on a further tie when i > j; the K best carry information. spec
 * receives the text in bchk_polar_design_bec's format (frozen symbols ascending; no shortening,
 * puncturing or dynamic freezing), err / soft (may be NULL) the U sums. 1 <= K <= U and
 * 1 <= words <= 2^31, else BCHK_EINVAL with nothing written; *needed and spec_len as in
 * bchk_polar_design_bec (a short buffer is BCHK_EINVAL with *needed set and nothing else
 * written). */
int bchk_polar_design_genie(const char *layers, const char *kdir, int K, double snr_db, uint64_t words,
                            uint64_t seed, int device, uint64_t *err, int64_t *soft, char *spec, size_t spec_len,
                            size_t *needed);
/* bchk_polar_genie_run and bchk_polar_design_genie with (channel, param) of
 * bchk_polar_generate_channel_device in place of snr_db: nothing in the genie-aided statistics is
 * specific to AWGN, only the source of the LLRs is, and a frozen set designed this way is a
 * design for the channel the decoder will see (for the BSC at crossover probability param). The
 * same refusals, and BCHK_EINVAL for an unknown channel or a p outside (0, 0.5], checked first;
 * BCHK_CHANNEL_AWGN gives the calls above exactly. */
int bchk_polar_genie_run_channel(bchk_polar *pc, int channel, double param, uint64_t words, uint64_t seed,
                                 uint64_t word0, size_t batch, uint64_t *err, int64_t *soft, double *seconds);
int bchk_polar_design_genie_channel(const char *layers, const char *kdir, int K, int channel, double param,
                                    uint64_t words, uint64_t seed, int device, uint64_t *err, int64_t *soft,
                                    char *spec, size_t spec_len, size_t *needed);
/* The same over a fading model: (kind, param) of bchk_polar_generate_fading_device, snr_db the
 * average Eb/N0. The same refusals, (kind, param) checked first. */
int bchk_polar_genie_run_fading(bchk_polar *pc, int kind, double param, double snr_db, uint64_t words,
                                uint64_t seed, uint64_t word0, size_t batch, uint64_t *err, int64_t *soft,
                                double *seconds);
int bchk_polar_design_genie_fading(const char *layers, const char *kdir, int K, int kind, double param,
                                   double snr_db, uint64_t words, uint64_t seed, int device, uint64_t *err,
                                   int64_t *soft, char *spec, size_t spec_len, size_t *needed);

const char *bchk_last_error(void);
const char *bchk_version(void);

#ifdef __cplusplus
}
#endif
#endif
