#!/usr/bin/env python3
"""Write tests/golden/long_mixed_ref_*.txt.gz: codes over extended-BCH kernels longer than the C
oracle takes (U > 4096), with the lists of the reference's own decoder (oracle/_ref/polar_ref,
built by `make -C oracle ref`). tests/test_polar_mixed_tiered.py decodes them with the tiered
mixed-kernel SC-list kernel. The format: tests/polar_ref_lib.py (@spec, @kernel, @llr,
@decode L); the kernel files are embedded as in the polar_ref_mixed_* fixtures.

The words are random information words through the reference's encoder, sent over AWGN at an
Eb/N0 where the list matters: the seed of a case is the first one at which some recorded row's
best path differs from the reference's own L = 1 decode of that row; the comment line names it.
A file may be no larger than the largest long_ref_* fixture.
"""
import glob
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import polar_ref_lib as R  # noqa: E402
from make_long_golden import MAX_SEEDS  # noqa: E402
from polar_lib import awgn_llr  # noqa: E402
from test_polar_mixed import KERNELS  # noqa: E402

CASES = [  # name, layers, K, dynamic constraints, L, rows, Eb/N0
    ("8192_4096_A_ebch16x3_L8", ("A", "bch16", "bch16", "bch16"), 4096, 6, 8, 2, 2.0),
    ("16384_8192_A2_ebch16x3_L4", ("A", "A", "bch16", "bch16", "bch16"), 8192, 0, 4, 1, 2.0),
]


def partial_distances(Km):
    """D_r: the least weight of row r plus any combination of the rows after it."""
    l = len(Km)
    rows = [int("".join(str(int(v)) for v in r), 2) for r in Km]
    out = []
    for r in range(l):
        best = l
        for v in range(1 << (l - 1 - r)):
            w = rows[r]
            for t in range(l - 1 - r):
                if (v >> t) & 1:
                    w ^= rows[r + 1 + t]
            best = min(best, bin(w).count("1"))
        out.append(best)
    return out


def spec_by_distance(layers, K, dyn, seed):
    """Specification text over the layers ("A" or a kernel of test_polar_mixed.KERNELS): symbol
    i = (i_0, ..., i_{nl-1}), the channel-side layer's digit first, is unfrozen when the product of
    the partial distances of its rows is among the K largest (ties: the larger index), the
    Reed-Muller rule; `dyn` frozen symbols are the XOR of two earlier ones."""
    mats = [np.array([[1, 0], [1, 1]], np.uint8) if n == "A" else KERNELS[n] for n in layers]
    score = np.ones(1)
    for Km in mats:
        score = np.multiply.outer(score, np.array(partial_distances(Km), float)).reshape(-1)
    U = len(score)
    order = sorted(range(U), key=lambda i: (score[i], i))
    frozen = sorted(order[:U - K])
    rng = np.random.default_rng(seed)
    cand = [f for f in frozen if f >= 2]
    dynset = set(rng.choice(cand, size=min(dyn, len(cand)), replace=False).tolist()) if dyn else set()
    lines = [f"{U} {K} 0 {len(layers)} 0 0", " ".join("A" if n == "A" else f"-{n}.txt" for n in layers)]
    for f in frozen:
        if f in dynset:
            a, b = sorted(rng.choice(f, size=2, replace=False).tolist())
            lines.append(f"3 {a} {b} {f}")
        else:
            lines.append(f"1 {f}")
    return "\n".join(lines) + "\n"


def attempt(name, spec, kernels, L, rows, snr, seed, d):
    """The fixture at `seed`, and the rows whose best path is not the L = 1 decode."""
    N, K = (int(v) for v in spec.split()[:2])
    info = np.random.default_rng(seed).integers(0, 2, (rows, K)).astype(np.uint8)
    cw = np.array([R.bits(r) for r in R.run_ref(["encode", "spec.txt"], [R.bits_row(w) for w in info], d)])
    llr = awgn_llr(cw, snr, K / N, seed=seed + 1)
    lines = [R.hex_row(r) for r in llr]
    fx = R.Fixture(name)
    fx.add("spec", [], spec.rstrip("\n").split("\n"))
    for kname in kernels:
        Km = KERNELS[kname]
        fx.add("kernel", [f"{kname}.txt", len(Km)], [" ".join(str(int(v)) for v in row) for row in Km])
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
    limit = max(os.path.getsize(p) for p in glob.glob(os.path.join(R.GOLD, "long_ref_*.txt.gz")))
    for i, (name, layers, K, dyn, L, rows, snr) in enumerate(CASES):
        spec = spec_by_distance(layers, K, dyn, seed=len(layers))
        kernels = sorted(set(n for n in layers if n != "A"))
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "spec.txt"), "w") as f:
                f.write(spec)
            for kname in kernels:
                with open(os.path.join(d, f"{kname}.txt"), "w") as f:
                    f.write(R.kernel_text(KERNELS[kname]))
            for seed in range(2000 + 100 * i, 2000 + 100 * i + MAX_SEEDS):
                fx, differ = attempt(name, spec, kernels, L, rows, snr, seed, d)
                if differ:
                    break
            else:
                sys.exit(f"{name}: no seed in {MAX_SEEDS} at {snr} dB where the list changes the best path")
        U = int(np.prod([2 if n == "A" else len(KERNELS[n]) for n in layers]))
        fx.comments = [f"long_mixed_ref fixture: ({U}, {K}) code over {' x '.join(layers)}, {dyn} dynamic constraints, "
                       f"L = {L}, Eb/N0 {snr:g} dB, seed {seed}; recorded lists of the reference's vendored decoder "
                       f"(scripts/make_long_mixed_golden.py). Rows whose best path differs from the reference's "
                       f"L = 1 decode: {differ}"]
        path = os.path.join(R.GOLD, f"long_mixed_ref_{name}.txt.gz")
        fx.save(path)
        size = os.path.getsize(path)
        print(os.path.basename(path), size, f"seed {seed}, rows {differ} differ from L = 1")
        if size > limit:
            sys.exit(f"{os.path.basename(path)}: {size} B exceeds the largest long_ref fixture ({limit} B): cut rows")


if __name__ == "__main__":
    main()
