#!/usr/bin/env python3
"""Write tests/golden/named_ref_*.txt.gz: codes over the library's named kernels G and A5, with
the outputs of the reference's own decoder and encoder (oracle/_ref/polar_ref, built by `make
-C oracle ref`). The cases and the format: tests/named_lib.py, tests/polar_ref_lib.py.

Every decode is run twice, with the C library's allocator filling fresh memory with two
different bytes (MALLOC_PERTURB_ = 1 and 200): the reference's G processor reads a state it
never copied when G sits in an outer layer of a list decode, and a case whose two
outputs differ is refused, never recorded.
"""
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import named_lib as NL  # noqa: E402
import polar_ref_lib as R  # noqa: E402
from bchk_pkg import load  # noqa: E402
from polar_lib import awgn_llr  # noqa: E402


def run_perturbed(args, lines, d):
    outs = []
    for fill in ("1", "200"):
        os.environ["MALLOC_PERTURB_"] = fill
        try:
            outs.append(R.run_ref(args, lines, d))
        finally:
            del os.environ["MALLOC_PERTURB_"]
    if outs[0] != outs[1]:
        sys.exit(f"polar_ref {args}: the output depends on uninitialised memory; not recorded")
    return outs[0]


def inputs(name, spec, kernels, lists, snr, seed, rows, ties=False, what="named kernels", large=None):
    fx = R.Fixture(name, [f"named_ref fixture: code {name} ({what}), Eb/N0 {snr:g} dB, seed {seed}; recorded outputs "
                          "of the reference's vendored decoder and encoder (scripts/make_named_golden.py)"])
    fx.add("spec", [], spec.rstrip("\n").split("\n"))
    for fname, K in kernels.items():
        fx.add("kernel", [fname, len(K)], [" ".join(str(int(v)) for v in r) for r in K])
    N, K = (int(v) for v in spec.split()[:2])
    rng = np.random.default_rng(seed)
    dec_info = rng.integers(0, 2, (rows, K)).astype(np.uint8)
    enc_info = rng.integers(0, 2, (NL.ENC_WORDS, K)).astype(np.uint8)
    with tempfile.TemporaryDirectory() as d:
        fx.write_kernels(d)
        with open(os.path.join(d, "spec.txt"), "w") as f:
            f.write(spec)
        cw = np.array([R.bits(r) for r in R.run_ref(["encode", "spec.txt"], [R.bits_row(w) for w in dec_info], d)])
    llr = awgn_llr(cw, snr, K / N, seed=seed + 1)
    if ties:  # equal metrics and exact zeros: multiples of 4 (|llr| < 2 becomes 0)
        llr = (4.0 * np.round(llr / 4.0)).astype(np.float32)
    if large:  # large magnitudes, still below a shortened symbol's 100000
        llr[rows // 2:] *= np.float32(large)
    fx.add("llr", [], [R.hex_row(r) for r in llr])
    for L in lists:
        fx.add("decode", [L], [])
    fx.add("info", [], [R.bits_row(w) for w in enc_info])
    fx.add("encode", [], [])
    return fx


def record(fx):
    """The fixture with its output sections computed, every decode under both fills."""
    out = R.Fixture(fx.name, fx.comments)
    with tempfile.TemporaryDirectory() as d:
        fx.write_kernels(d)
        with open(os.path.join(d, "spec.txt"), "w") as f:
            f.write(fx.spec)
        for n, a, lines in fx.sections:
            if n == "decode":
                lines = run_perturbed(["decode", "spec.txt", a[0]], fx.get("llr"), d)
            elif n == "encode":
                lines = run_perturbed(["encode", "spec.txt"], fx.get("info"), d)
            out.sections.append((n, a, lines))
    return out


def save(fx):
    path = os.path.join(R.GOLD, f"named_ref_{fx.name}.txt.gz")
    fx.save(path)
    print(os.path.basename(path), os.path.getsize(path))


def shortened_symbol_is_zero(spec, short):
    """The shortened symbols of the code's unshortened codewords are zero for every word."""
    lines = spec.rstrip("\n").split("\n")
    N, K, dmin, nl, nsh, npu = (int(v) for v in lines[0].split())
    full = "\n".join([f"{N + nsh + npu} {K} {dmin} {nl} 0 0", lines[1]] + lines[3:]) + "\n"
    rng = np.random.default_rng(5)
    words = rng.integers(0, 2, (64, K)).astype(np.uint8)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "spec.txt"), "w") as f:
            f.write(full)
        cw = np.array([R.bits(r) for r in R.run_ref(["encode", "spec.txt"], [R.bits_row(w) for w in words], d)])
    return not cw[:, list(short)].any()


def main():
    if not os.path.exists(R.POLAR_REF):
        sys.exit("build the reference first: make -C oracle ref")
    F = load()
    kern = {"-bch8.txt": F.kernel_ebch(3), "-G.txt": NL.G}
    for p in NL.named_files() + NL.outer_files():
        os.remove(p)
    for i, (name, layers, K, lists, ex) in enumerate(NL.CASES):
        U = int(np.prod([NL.SIZES[n] for n in layers]))
        seed = 100 + 13 * i
        spec = NL.named_spec(layers, K, seed, ex.get("dyn", 0), ex.get("punct", ()), ex.get("short", ()),
                             ex.get("freeze", ()))
        if ex.get("short"):
            assert shortened_symbol_is_zero(spec, ex["short"]), name
        kernels = {n[1:]: kern[n] for n in layers if n.startswith("-")}
        snr = 1.0 + 0.25 * np.log2(U)
        save(record(inputs(name, spec, kernels, lists, snr, seed, NL.ROWS, ties=bool(ex.get("ties")), large=ex.get("large"))))
    # G in an outer layer with a list: the matrix form of the code, close metrics dropped
    for i, (name, layers, K, lists) in enumerate(NL.OUTER_CASES):
        for seed in range(700 + 10 * i, 710 + 10 * i):
            spec = NL.named_spec(layers, K, seed)
            fx = record(inputs(name, spec, {"G.txt": NL.G}, lists, 2.0, seed, NL.OUTER_ROWS,
                               what="matrix form -G.txt of an outer G layer"))
            keep = [b for b in range(NL.OUTER_ROWS)
                    if all(NL.list_metric_gap(fx.decoded(L)[b][3]) >= NL.OUTER_GAP for L in lists)]
            if len(keep) >= (1.0 - NL.OUTER_MAX_DROP) * NL.OUTER_ROWS:
                break
            print(f"{name}: seed {seed} would drop {NL.OUTER_ROWS - len(keep)} rows, next seed")
        else:
            sys.exit(f"{name}: no seed keeps {100 * (1 - NL.OUTER_MAX_DROP):g} % of the rows")
        llr = fx.get("llr")
        kept = R.Fixture(fx.name, fx.comments + [f"rows kept: {len(keep)} of {NL.OUTER_ROWS} (a row with two list metrics "
                                                 "closer than 2^-18 relative is dropped)"])
        for n, a, lines in fx.sections:
            kept.sections.append((n, a, [llr[b] for b in keep] if n == "llr" else [] if n in ("decode", "encode") else lines))
        save(record(kept))


if __name__ == "__main__":
    main()
