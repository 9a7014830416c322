#!/usr/bin/env python3
"""Write tests/golden/long_ref_*.txt.gz: all-Arikan codes longer than the C oracle takes (U >
4096), with the lists of the reference's own decoder (oracle/_ref/polar_ref, built by `make -C
oracle ref`). tests/test_polar_tiered.py decodes them with the tiered SC-list kernel. The
format: tests/polar_ref_lib.py (@spec, @llr, @decode L).

The words are random information words through the reference's encoder, sent over AWGN at an
Eb/N0 where the list matters: the seed of a case is the first one at which some recorded row's
best path differs from the reference's own L = 1 decode of that row; the comment line names it.
"""
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import polar_ref_lib as R  # noqa: E402
from polar_lib import arikan_spec, awgn_llr  # noqa: E402

CASES = [  # name, n, K, dynamic constraints, punctured symbols, L, rows, Eb/N0
    ("8192_4096_dyn6_L8", 13, 4096, 6, (), 8, 2, 1.5),
    ("16384_8192_L4", 14, 8192, 0, (), 4, 2, 1.5),
    ("16384_8192_L32", 14, 8192, 0, (), 32, 1, 1.5),
    ("16381_8192_punct3_L8", 14, 8192, 0, (5, 4097, 16000), 8, 1, 1.5),
]
MAX_SEEDS = 40


def attempt(name, spec, L, rows, snr, seed, d):
    """The fixture at `seed`, and the rows whose best path is not the L = 1 decode."""
    N, K = (int(v) for v in spec.split()[:2])
    info = np.random.default_rng(seed).integers(0, 2, (rows, K)).astype(np.uint8)
    cw = np.array([R.bits(r) for r in R.run_ref(["encode", "spec.txt"], [R.bits_row(w) for w in info], d)])
    llr = awgn_llr(cw, snr, K / N, seed=seed + 1)
    lines = [R.hex_row(r) for r in llr]
    fx = R.Fixture(name)
    fx.add("spec", [], spec.rstrip("\n").split("\n"))
    fx.add("llr", [], lines)
    fx.add("decode", [L], R.run_ref(["decode", "spec.txt", L], lines, d))
    one = R.Fixture(name)
    one.add("decode", [1], R.run_ref(["decode", "spec.txt", 1], lines, d))
    best, sc = fx.decoded(L), one.decoded(1)
    differ = [b for b in range(rows) if not np.array_equal(best[b][1][0], sc[b][1][0])]
    return fx, differ


def main():
    if not os.path.exists(R.POLAR_REF):
        sys.exit("build the reference first: make -C oracle ref")
    for i, (name, n, K, dyn, punct, L, rows, snr) in enumerate(CASES):
        spec = arikan_spec(n, K, dyn=dyn, punct=punct, seed=n)
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "spec.txt"), "w") as f:
                f.write(spec)
            for seed in range(1000 + 100 * i, 1000 + 100 * i + MAX_SEEDS):
                fx, differ = attempt(name, spec, L, rows, snr, seed, d)
                if differ:
                    break
            else:
                sys.exit(f"{name}: no seed in {MAX_SEEDS} at {snr} dB where the list changes the best path")
        fx.comments = [f"long_ref fixture: ({(1 << n) - len(punct)}, {K}) Arikan code, {dyn} dynamic constraints, "
                       f"punctured {list(punct)}, L = {L}, Eb/N0 {snr:g} dB, seed {seed}; recorded lists of the "
                       f"reference's vendored decoder (scripts/make_long_golden.py). Rows whose best path differs "
                       f"from the reference's L = 1 decode: {differ}"]
        path = os.path.join(R.GOLD, f"long_ref_{name}.txt.gz")
        fx.save(path)
        print(os.path.basename(path), os.path.getsize(path), f"seed {seed}, rows {differ} differ from L = 1")


if __name__ == "__main__":
    main()
