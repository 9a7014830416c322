#!/usr/bin/env python3
"""oracle/make_golden.py -- TEST INFRASTRUCTURE ONLY.

Regenerates the golden fixtures under tests/golden/ by RUNNING THE REFERENCE ITSELF:
oracle/_ref/ref_golden and oracle/_ref/kaneko are compiled by oracle/Makefile from the
unmodified sources under /root/reference (this container only). The fixtures are data
(inputs and the reference's outputs); no reference source text is stored.

    make -C oracle ref && python oracle/make_golden.py            # the Kaneko fixtures
    make -C oracle ref && python oracle/make_golden.py polar      # the polar_ref_* fixtures
    make -C oracle ref && python oracle/make_golden.py polar-lists  # polar_ref_lists_* alone

The `polar` sub-command needs the product library built as well (kernel matrices come from
its bchk_kernel_ebch): oracle/_ref/polar_ref is our driver (oracle/polar_ref.cpp) linked with
the reference's vendored polar library. The polar_ref_*.txt.gz format is described in
tests/polar_ref_lib.py.

Fixture formats (gzip text, one record per line):
  vectors_*.txt.gz, vecj15_*.txt.gz (the J = 15 build)
                     '# code n k t m gsize G seed S snr X count C' header, then per word
                     'W <tx bits> <y_0..y_{n-1} as %a> <res bits | -> <l0 %a> <decodes>
                      <comparisons> <sums> <accepted>'  (src/KanekoKernelProcessor.cpp:335)
  infile_m6t6.txt    the in/infile.txt known answer, same 'W' line (counters absolute)
  algdec_*.txt.gz    'A <word bits> <ok> <answer bits | ->'  (src/Decoder.cpp:298)
  sweep_*.csv        the reference CLI `kaneko m t file p e` output (src/dataForPlot.cpp:80)
  cli_*.txt          stdout of the reference CLI modes 1 and 3 (src/main.cpp:100-172)
  infile_input.txt   the reference's in/infile.txt fixture (input data of mode 3)
"""
import gzip
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(REPO, "tests", "golden")
REF = os.path.join(HERE, "_ref")

# (m, t, seed, count, snr_db). J = infinity (the shipped build). Seeds vary the stream.
VECTORS = [
    (4, 2, 1, 256, 0.0), (4, 2, 7, 256, 3.0),
    (5, 3, 1, 256, 1.0), (5, 3, 11, 256, 4.0),
    (6, 6, 1, 128, 4.0), (6, 6, 13, 192, 4.5), (6, 6, 17, 256, 5.0), (6, 6, 19, 256, 6.0),
    (8, 15, 1, 48, 6.0), (8, 15, 23, 48, 7.0),
    # the lowest and the top t of the small (m, TMAX) kernel sets (select_kernels), and codes
    # of one information bit ((3,2), (3,3), (4,4), (4,7)), of 2t + 1 = n ((3,3), (4,7)) and of a
    # true distance above the designed one ((5,4): the generator of (5,5))
    (2, 1, 5, 64, 3.0),
    (3, 1, 5, 64, 3.0), (3, 2, 5, 64, 3.0), (3, 3, 5, 64, 3.0),
    (4, 1, 5, 64, 3.0), (4, 3, 5, 64, 3.0), (4, 4, 5, 64, 3.0), (4, 7, 5, 32, 3.0),
    (5, 1, 5, 64, 4.0), (5, 4, 5, 64, 4.0), (5, 6, 5, 64, 4.0),
]
# The same with the J = 15 build (oracle/_ref/ref_golden_j15): files vecj15_*, which
# vectors_*'s readers (J = infinity) do not match. Lowest and top t of every remaining kernel
# set. Every fixture of a set with TMAX > 8 holds at least two words of more than 8 * 64
# decodes (past chunk_limit, where the cooperative kernel takes over), except (5,15): of this
# repetition code with 2t + 1 = n no word took more than 512 decodes in 20 000 reference words
# at each of -20, -10, -5, 0 and 5 dB, 40 000 at -60 and -40 dB and 60 000 at -30 dB (maximum
# 481, at -30 dB), so the condition is unmet there; it is recorded at a noisy point and the
# hand-off of its kernel set is covered by (5,9) .. (5,12).
# (6,31), the other such code, passes 512 decodes in about one word of 800 at -12 dB (6 of 4096
# words of seeds 1 .. 8; maximum 2134): seed 244 is the first of seeds 1 .. 900 whose first 32
# words hold two of them (words 13 and 24).
# <7,32>: the reference did not finish 16 words of (7,32) in 25 s at 11, 13 or 15 dB (nor at
# 7 or 9 dB), so t = 32 is pinned by the algebraic-decoder fixture alone and the Kaneko
# fixtures of the set are t = 17 and t = 31.
VECTORS_J15 = [
    (5, 8, 5, 32, 4.0), (5, 9, 5, 32, 4.0), (5, 15, 5, 64, -10.0),
    (6, 1, 5, 32, 5.0), (6, 7, 5, 32, 3.0), (6, 12, 5, 32, 5.0), (6, 13, 5, 32, 5.0), (6, 31, 244, 32, -12.0),
    (7, 1, 5, 16, 4.0), (7, 8, 5, 16, 3.5), (7, 9, 5, 16, 3.5), (7, 16, 5, 16, 5.5), (7, 17, 5, 16, 5.5),
    (7, 31, 5, 16, 8.0),
    (8, 1, 5, 16, 2.0), (8, 16, 5, 16, 4.5), (8, 17, 5, 16, 4.0), (8, 32, 5, 16, 7.5),
]
ALGDEC = [(4, 2, "exhaustive", 0, 0), (5, 3, "exhaustive", 0, 0),
          (6, 6, "random", 20000, 31), (8, 15, "random", 3000, 37),
          (2, 1, "exhaustive", 0, 0), (3, 1, "exhaustive", 0, 0), (3, 3, "exhaustive", 0, 0),
          (4, 3, "exhaustive", 0, 0),
          (5, 15, "random", 2500, 41), (6, 12, "random", 2500, 43), (6, 31, "random", 2500, 47),
          (7, 16, "random", 2500, 53), (7, 32, "random", 2500, 59), (8, 16, "random", 2000, 61),
          (8, 32, "random", 2000, 67)]
SWEEPS = [(4, 2, 10000, 10000), (5, 3, 10000, 100)]


def run(args, cwd=None):
    return subprocess.run(args, check=True, capture_output=True, text=True, cwd=cwd).stdout


def vector_jobs():
    """(fixture file name, reference command) of every Kaneko vectors fixture."""
    jobs = []
    for exe, prefix, rows in (("ref_golden", "vectors", VECTORS), ("ref_golden_j15", "vecj15", VECTORS_J15)):
        for m, t, seed, count, snr in rows:
            jobs.append((f"{prefix}_m{m}t{t}_s{seed}_snr{snr:g}.txt.gz",
                         [os.path.join(REF, exe), "vectors", str(m), str(t), str(seed), str(count), repr(snr)]))
    return jobs


def algdec_jobs():
    """(fixture file name, reference command) of every algebraic-decoder fixture."""
    return [(f"algdec_m{m}t{t}_{what}.txt.gz",
             [os.path.join(REF, "ref_golden"), "algdec", str(m), str(t), what, str(count), str(seed)])
            for m, t, what, count, seed in ALGDEC]


def kaneko():
    if not all(os.path.exists(os.path.join(REF, exe)) for exe in ("ref_golden", "ref_golden_j15")):
        sys.exit("build the reference first: make -C oracle ref")
    os.makedirs(GOLD, exist_ok=True)
    for name, args in vector_jobs() + algdec_jobs():
        out = run(args)
        with gzip.open(os.path.join(GOLD, name), "wt") as f:
            f.write(out)
        print(name, len(out))
    out = run([os.path.join(REF, "ref_golden"), "file", "6", "6",
               "/root/reference/in/infile.txt"])
    with open(os.path.join(GOLD, "infile_m6t6.txt"), "w") as f:
        f.write(out.replace("/root/reference/in/infile.txt", "in/infile.txt"))
    # CLI modes 1 and 3 of src/main.cpp (stdout), and the mode-3 input itself (data)
    for args, name in ((["6", "6", "0.0", "/root/reference/in/infile.txt"], "cli_infile_m6t6.txt"),
                       (["6", "6", "3.0"], "cli_random_m6t6_snr3.txt"),
                       (["4", "2", "4.0"], "cli_random_m4t2_snr4.txt")):
        with open(os.path.join(GOLD, name), "w") as f:
            f.write(run([os.path.join(REF, "kaneko")] + args))
    with open("/root/reference/in/infile.txt") as src, \
            open(os.path.join(GOLD, "infile_input.txt"), "w") as dst:
        dst.write(src.read())
    tmp = os.path.join(REF, "sweep_tmp")
    os.makedirs(tmp, exist_ok=True)
    for m, t, p, e in SWEEPS:
        run([os.path.join(REF, "kaneko"), str(m), str(t), "out", str(p), str(e)], cwd=tmp)
        name = f"sweep_m{m}t{t}_p{p}_e{e}.csv"
        with open(os.path.join(tmp, "out.csv")) as src, open(os.path.join(GOLD, name), "w") as dst:
            dst.write(src.read())
        print(name)


# ------------------------------------------------------------------------ polar fixtures
# Arikan codes: n, K, dynamic frozen, punctured, list sizes (test_polar_sclist's codes; for
# n = 3, 4 the lists of 8 and 32 are the full 2^K lists). Eb/N0 = 1.0 + 0.25 n dB.
POLAR_LISTS = (1, 2, 4, 8, 32)
POLAR_ARIKAN = [(3, 3, 0, ()), (4, 5, 0, ()), (5, 16, 3, ()), (6, 32, 5, (1, 7)),
                (8, 128, 12, (0, 3, 17, 40))]
# matrix-kernel codes: layers (outermost first), K, dynamic frozen, punctured
POLAR_MIXED = [(("k4", "A"), 4, 0, ()), (("bch8", "A"), 8, 2, ()), (("bch16", "A"), 16, 2, ()),
               (("bch32f",), 16, 2, ()), (("bch32f", "A"), 32, 2, ())]
# bch32f: the 32 x 32 extended-BCH kernel in field-element column order (bchk_kernel_field_order,
# the reference's swapColumns). As bchk_kernel_ebch leaves it its trellis has 2^13 states, over
# the GPU decoder's 2^12: that form is pinned by its trellis fixture (trellis_bch32) alone.
POLAR_MIXED_LISTS = (1, 4, 8)
POLAR_WORDS = 32
# shortened codes (the decoder's 100000 at a shortened symbol): tests/test_polar_contract.py's
# specifications of these names -- A^6 with five shortened symbols, eBCH16 x A with three, A^7
# shortened, punctured and dynamically frozen -- at 0 dB, where the lists diverge, the upper half
# of the rows times 4096: with LLRs of order 1 alone no list depends on the mapped value as long as
# it is the largest (tests/short_codes.py: FIXTURES, with_large_rows)


# list sizes that are no power of two (tests/test_polar_list_sizes.py): four codes, every L of
# POLAR_ODD_LISTS each. `polar-lists` writes these files and touches no other.
POLAR_ODD_LISTS = (3, 5, 6, 7, 12, 24, 31)


def polar_lists(code_fixture, emit):
    import numpy as np

    import dense_codes
    from polar_lib import arikan_spec
    from test_polar_mixed import mixed_spec

    emit(code_fixture("lists_arikan_n6", arikan_spec(6, 32, dyn=5, punct=(1, 7), seed=6), (), POLAR_ODD_LISTS,
                      1.0 + 0.25 * 6, seed=606))
    # the arikan_n7_ties recipe: LLRs rounded to multiples of 4 (|llr| < 2 becomes 0)
    emit(code_fixture("lists_arikan_n7_ties", arikan_spec(7, 64, dyn=4, seed=77), (), POLAR_ODD_LISTS, 1.0, seed=707,
                      llr_map=lambda x: (4.0 * np.round(x / 4.0)).astype(np.float32)))
    # a matrix kernel, which the reference takes through its trellis processor
    emit(code_fixture("lists_bch8_A", mixed_spec(("bch8", "A"), 8, 2, (), seed=2 * 11 + 8), ["bch8"], POLAR_ODD_LISTS,
                      1.0 + 0.25 * 4, seed=808))
    # 33 constraints live at once: bit 32, in the upper half of the mask. 28 words: with 32 the file
    # is larger than the largest other polar_ref_* fixture (arikan_n8)
    name = "dyn_arikan_n7_a33"
    emit(code_fixture("lists_" + name, dense_codes.spec(name), (), POLAR_ODD_LISTS, dense_codes.SNR[name], seed=909,
                      words=28))


def polar(lists_only=False):
    import tempfile

    import numpy as np

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import polar_ref_lib as R
    from bchk_pkg import load
    from polar_lib import arikan_spec, awgn_llr
    from test_polar_mixed import KERNELS, mixed_spec

    if not os.path.exists(R.POLAR_REF):
        sys.exit("build the reference first: make -C oracle ref")
    F = load()
    kern = {"k4": KERNELS["k4"], "bch8": F.kernel_ebch(3), "bch16": F.kernel_ebch(4), "bch32": F.kernel_ebch(5),
            "bch32f": F.kernel_field_order(5, F.kernel_ebch(5))}
    os.makedirs(GOLD, exist_ok=True)
    if not lists_only:
        for p in sum((R.fixture_files(k) for k in ("code", "trellis", "counts", "capacity")), []):
            os.remove(p)

    def emit(fx):
        with tempfile.TemporaryDirectory() as d:
            out = R.regenerate(fx, d)
        path = os.path.join(GOLD, f"polar_ref_{fx.name}.txt.gz")
        out.save(path)
        print(os.path.basename(path), os.path.getsize(path))

    def code_fixture(name, spec, kernels, lists, snr, seed, llr_map=None, words=POLAR_WORDS):
        """Inputs of one code: random information words, their codewords (by the reference's own
        encoder) over BPSK / AWGN at Eb/N0 snr."""
        fx = R.Fixture(name, [f"polar_ref fixture: code {name}, Eb/N0 {snr:g} dB, seed {seed}; recorded outputs of "
                              "the reference's vendored decoder and encoder (oracle/make_golden.py polar)"])
        fx.add("spec", [], spec.rstrip("\n").split("\n"))
        for kname in kernels:
            fx.add("kernel", [f"{kname}.txt", len(kern[kname])], [" ".join(str(int(v)) for v in r) for r in kern[kname]])
        hdr = [int(v) for v in spec.split()[:6]]
        N, K = hdr[0], hdr[1]
        rng = np.random.default_rng(seed)
        dec_info = rng.integers(0, 2, (words, K)).astype(np.uint8)
        enc_info = rng.integers(0, 2, (30, K)).astype(np.uint8)
        with tempfile.TemporaryDirectory() as d:
            fx.write_kernels(d)
            with open(os.path.join(d, "spec.txt"), "w") as f:
                f.write(spec)
            cw = np.array([R.bits(r) for r in R.run_ref(["encode", "spec.txt"], [R.bits_row(w) for w in dec_info], d)])
        llr = awgn_llr(cw, snr, K / N, seed=seed + 1)
        if llr_map:
            llr = llr_map(llr)
        fx.add("llr", [], [R.hex_row(r) for r in llr])
        for L in lists:
            fx.add("decode", [L], [])
        fx.add("info", [], [R.bits_row(w) for w in enc_info])
        fx.add("encode", [], [])
        return fx

    polar_lists(code_fixture, emit)
    if lists_only:
        return
    for n, K, dyn, punct in POLAR_ARIKAN:
        emit(code_fixture(f"arikan_n{n}", arikan_spec(n, K, dyn=dyn, punct=punct, seed=n), (), POLAR_LISTS,
                          1.0 + 0.25 * n, seed=n * 7))
    # equal metrics and exact zeros: LLRs rounded to multiples of 4 (|llr| < 2 becomes 0)
    emit(code_fixture("arikan_n7_ties", arikan_spec(7, 64, dyn=4, seed=77), (), (8,), 1.0, seed=77,
                      llr_map=lambda x: (4.0 * np.round(x / 4.0)).astype(np.float32), words=48))
    for layers, K, dyn, punct in POLAR_MIXED:
        spec = mixed_spec(layers, K, dyn, punct, seed=len(layers) * 11 + K)  # sizes by test_polar_mixed's names
        U = int(np.prod([2 if l == "A" else len(kern[l]) for l in layers]))
        nbits = int(round(np.log2(U)))
        emit(code_fixture("mixed_" + "_".join(layers), spec, [l for l in layers if l != "A"], POLAR_MIXED_LISTS,
                          1.0 + 0.25 * nbits, seed=U + K))
    import short_codes
    with tempfile.TemporaryDirectory() as kd:
        short_codes.write_kernels(kd)
        for i, name in enumerate(short_codes.FIXTURES):
            emit(code_fixture("short_" + name, short_codes.short_spec(name, kd), ["bch16"] if "bch16" in name else [],
                              POLAR_MIXED_LISTS, 0.0, seed=900 + i, llr_map=short_codes.with_large_rows))
    # dense dynamic freezing (tests/dense_codes.py): 64, 33 and 40 constraints live at once, the
    # last code with constraints of 65 and 130 terms
    import dense_codes
    for i, name in enumerate(dense_codes.FIXTURES):
        emit(code_fixture(name, dense_codes.spec(name), [l for l in dense_codes.layers(name) if l != "A"],
                          POLAR_MIXED_LISTS, dense_codes.SNR[name], seed=2000 + i))
    for kname in ("bch8", "bch16", "bch32", "bch32f"):
        l = len(kern[kname])
        rng = np.random.default_rng(l + len(kname))
        fx = R.Fixture(f"trellis_{kname}", [f"polar_ref fixture: CTrellisKernelProcessor::GetLLRs of the {l} x {l} "
                                            "extended-BCH kernel, every phase (oracle/make_golden.py polar)"])
        fx.add("kernel", [f"{kname}.txt", l], [" ".join(str(int(v)) for v in r) for r in kern[kname]])
        fx.add("trellis_in", [], [R.bits_row(rng.integers(0, 2, l)) + " " +
                                  R.hex_row(rng.normal(0, 1.5, l).astype(np.float32)) for _ in range(16)])
        fx.add("trellis_out", [], [])
        emit(fx)
    polar_counts(F, kern, emit)
    polar_capacity(F, emit)


# The column search's score (root bchCoder.cpp:641-653): SumCount / CmpCount growth over GetLLRs
# at every phase. Kernels: the extended-BCH kernels as built and in field-element order, Kronecker
# powers of the Arikan kernel, zero span (identity) and maximal span (identity, columns reversed),
# random invertible kernels of sizes that are no power of two, and the field-ordered 16 x 16
# kernel under five L.U column maps (the all-zero code, the all-one code, three seeded ones).
COUNT_RANDOM = (3, 5, 6, 7, 12)
COUNT_LU_CODES = (0, (1 << 12) - 1) + tuple(int(c) for c in __import__("numpy").random.default_rng(16).choice((1 << 12) - 2, 3, replace=False) + 1)


def polar_counts(F, kern, emit):
    import numpy as np

    import polar_ref_lib as R
    from test_kernel_search import llrs_like_reference, o_perm, rand_invertible

    F2 = np.array([[1, 0], [1, 1]], np.uint8)
    ks = {}
    for power in (2, 3, 4, 5):
        K = F.kernel_ebch(power)
        ks[f"bch{1 << power}"] = K
        ks[f"bch{1 << power}f"] = F.kernel_field_order(power, K)
    K = np.ones((1, 1), np.uint8)
    for k in (1, 2, 3, 4):
        K = np.kron(K, F2)
        ks[f"kron{k}"] = K
    ks["id8"] = np.eye(8, dtype=np.uint8)
    ks["rev8"] = np.eye(8, dtype=np.uint8)[:, ::-1]
    for l in COUNT_RANDOM:
        ks[f"rand{l}"] = rand_invertible(l, np.random.default_rng(1000 + l))
    for code in COUNT_LU_CODES:
        ks[f"bch16f_lu{code}"] = ks["bch16f"][:, o_perm(4, code)]
    refused = []
    for name, K in ks.items():
        l = len(K)
        fx = R.Fixture(f"counts_{name}", [f"polar_ref fixture: SumCount / CmpCount of CTrellisKernelProcessor::GetLLRs over every "
                                          f"phase of the {l} x {l} kernel {name}, zero known inputs (oracle/make_golden.py polar)"])
        fx.add("kernel", [f"{name}.txt", l], [" ".join(str(int(v)) for v in r) for r in K])
        if "_lu" in name:
            fx.add("lu_code", [name.split("_lu")[1]], [])
        rows = [llrs_like_reference(l, 31 * l + s) for s in range(3)]  # (rand() % 10) - 5: exact zeros occur
        rows += [np.zeros(l, np.float32), -(1 + np.arange(l) % 5).astype(np.float32)]
        fx.add("counts_in", [], [R.hex_row(r) for r in rows])
        fx.add("counts_out", [], [])
        try:
            emit(fx)
        except RuntimeError as e:
            refused.append((name, str(e)))
    print("kernels the reference refused:", refused or "none")


CAPACITIES = [round(0.05 * i, 2) for i in range(1, 20)] + [1 - 1e-9, 1.0, 1e-3, 1e-5, 1e-10, 1e-20, 1e-40, 0.0]


def polar_capacity(F, emit):
    """The library's kernel-file reader and BEC capacity evaluator on files bchk_kernel_write_file
    wrote (host only): exact tables of the 4 x 4 and 16 x 16 extended-BCH kernels from the numpy
    checker, and of the 5-fold Kronecker power of the Arikan kernel from its closed form."""
    import tempfile

    import numpy as np

    import polar_ref_lib as R
    from test_kernel_bec import kron_power_table
    from test_polar_design import F2, table_of

    K5 = F2
    for _ in range(4):
        K5 = np.kron(K5, F2)
    cases = [("bch4", "k4t.txt", F.kernel_ebch(2), None), ("bch16", "e16t.txt", F.kernel_ebch(4), None),
             ("kron5", "f32t.txt", K5, np.array(kron_power_table(5), np.uint64))]
    for name, fname, K, tab in cases:
        tab = table_of(K) if tab is None else tab
        with tempfile.TemporaryDirectory() as d:
            F.write_kernel_file(os.path.join(d, fname), K, tab)
            text = open(os.path.join(d, fname)).read()
        assert text.endswith("\n")
        fx = R.Fixture(f"capacity_{name}", [f"polar_ref fixture: CMatrixBinaryKernel's reader and CBECCapacityEvaluator::"
                                            f"GetSubchannelCapacity on the file bchk_kernel_write_file wrote for {name} "
                                            "(oracle/make_golden.py polar)"])
        fx.add("kernel_file", [fname], text[:-1].split("\n"))
        fx.add("capacity_in", [], [R.hex64(c) for c in CAPACITIES])
        fx.add("capacity_out", [], [])
        emit(fx)


def main():
    import argparse
    ap = argparse.ArgumentParser(
        description="Regenerate tests/golden/ by running the compiled reference (oracle/_ref/, built by "
                    "`make -C oracle ref`).",
        epilog="`python oracle/make_golden.py` rewrites the Kaneko fixtures; `python oracle/make_golden.py polar` "
               "rewrites every polar_ref_*.txt.gz (SC-list decoder, encoder, trellis kernel processor, its "
               "operation counts, the BEC capacity evaluator); `python oracle/make_golden.py polar-lists` writes the "
               "polar_ref_lists_*.txt.gz among them and leaves the others as they are.")
    ap.add_argument("what", nargs="?", default="kaneko", choices=["kaneko", "polar", "polar-lists"])
    {"kaneko": kaneko, "polar": polar, "polar-lists": lambda: polar(lists_only=True)}[ap.parse_args().what]()


if __name__ == "__main__":
    main()
