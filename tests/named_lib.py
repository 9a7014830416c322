"""The tests/golden/named_ref_*.txt.gz fixtures: codes over the library's named kernels G (3 x 3)
and A5 (5 x 5) (out/external/TruncatedArikanKernel.cpp), with the RECORDED OUTPUTS of the
reference's own decoder and encoder (oracle/_ref/polar_ref). Written by
scripts/make_named_golden.py, read by tests/test_polar_named_kernels.py; the format is
polar_ref_lib's. Data only.

Two groups:
  named_ref_<code>        the specification names G / A5; every recorded list size is one at
                          which the reference is defined (with a list, its G
                          state survives a path clone only when G is the innermost layer).
  named_ref_outerG_<code> G in an outer layer with a list. '@spec' and the recorded lists are
                          the MATRIX form of the same code (G given as the file -G.txt), which
                          the reference decodes through its trellis and is defined; the test
                          decodes the named form (named_form()). Rows with two list metrics
                          closer than 2^-18 relative were dropped when recording.
"""
import glob
import os

import numpy as np

import polar_ref_lib as R

G = np.array([[1, 0, 0], [1, 1, 0], [0, 1, 1]], np.uint8)
# what CA5Kernel::Multiply computes (the matrix of the file's comment, :193-197)
A5 = np.array([[1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 0, 1, 0, 0], [1, 0, 0, 0, 1], [1, 1, 1, 1, 0]], np.uint8)
SIZES = {"A": 2, "G": 3, "A5": 5, "-bch8.txt": 8, "-G.txt": 3}

ROWS, OUTER_ROWS, ENC_WORDS = 16, 64, 16
OUTER_GAP = 2.0 ** -18
OUTER_MAX_DROP = 0.02

# name, layers, K, list sizes, extras
CASES = [
    ("G", ("G",), 2, (1,), {}),
    ("A5", ("A5",), 3, (1, 4, 8), {}),
    ("A_G", ("A", "G"), 3, (1, 4), {}),
    ("A_A_G", ("A", "A", "G"), 6, (1, 4, 8), {}),
    ("A_A_A_A_A_G", ("A", "A", "A", "A", "A", "G"), 48, (1, 8, 32), {}),
    ("A5_A", ("A5", "A"), 5, (1, 4, 8), {}),
    ("A_A5", ("A", "A5"), 5, (1, 4, 8), {}),
    ("A_A5_A", ("A", "A5", "A"), 10, (1, 4, 8), {}),
    ("A5_A5", ("A5", "A5"), 12, (1, 4, 8), {}),
    ("A5_G", ("A5", "G"), 8, (1, 4, 8), {}),
    ("G_A", ("G", "A"), 3, (1,), {}),
    ("G_G", ("G", "G"), 5, (1,), {}),
    ("A_G_A", ("A", "G", "A"), 6, (1,), {}),
    ("G_A5", ("G", "A5"), 8, (1,), {}),
    # u_57 = digits (1, 2, 3, 1) is the only input that reaches codeword symbol 59 = (1, 2, 4, 1):
    # frozen, so the shortened symbol is always 0
    ("A_G_A5_A", ("A", "G", "A5", "A"), 30, (1,), {"dyn": 2, "punct": (0, 7), "short": (59,), "freeze": (57,)}),
    ("bch8_G", ("-bch8.txt", "G"), 12, (1, 8), {}),
    ("A_A5_A_ties", ("A", "A5", "A"), 10, (8,), {"ties": True}),
    ("A_A_G_ties", ("A", "A", "G"), 6, (8,), {"ties": True}),
    # u_29, the last input, frozen: symbol 11 is then always 0. G is not the innermost layer, so L = 1
    # only; the upper half of the LLR rows times 4096, magnitudes that only a mapped value of the
    # reference's size (100000 at the shortened symbol) still outweighs in every min
    ("A5_G_A_short", ("A5", "G", "A"), 14, (1,), {"short": (11,), "freeze": (29,), "large": 4096.0}),
]
OUTER_CASES = [("outerG_G_A_A", ("-G.txt", "A", "A"), 9, (4, 8)), ("outerG_A_G_A", ("A", "-G.txt", "A"), 9, (4, 8))]


def named_files():
    all_ = sorted(glob.glob(os.path.join(R.GOLD, "named_ref_*.txt.gz")))
    return [p for p in all_ if "named_ref_outerG_" not in p]


def outer_files():
    return sorted(glob.glob(os.path.join(R.GOLD, "named_ref_outerG_*.txt.gz")))


def ident(path):
    return os.path.basename(path)[len("named_ref_"):-len(".txt.gz")]


_fx = {}


def fixture(path):
    if path not in _fx:
        _fx[path] = R.load_fixture(path)  # ('named_ref_' is as long as 'polar_ref_': the name is the code's)
    return _fx[path]


def named_form(spec):
    """The specification with the matrix file -G.txt replaced by the named kernel."""
    lines = spec.split("\n")
    lines[1] = " ".join("G" if n == "-G.txt" else n for n in lines[1].split())
    return "\n".join(lines)


def named_spec(layers, K, seed, dyn=0, punct=(), short=(), freeze=()):
    """Specification text (MixedKernelEncoder.cpp:7-98) over the given layer names: the U - K
    lowest indices frozen but for a few swaps near the boundary, `freeze` frozen whatever its
    rank, `dyn` frozen symbols dynamic (the XOR of two earlier symbols)."""
    U = int(np.prod([SIZES[n] for n in layers]))
    rng = np.random.default_rng(seed)
    order = [i for i in range(U) if i not in freeze]
    lo, hi = max(0, U - K - 4), min(len(order), U - K + 4)
    for _ in range(max(1, U // 8)):
        i, j = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        order[i], order[j] = order[j], order[i]
    frozen = sorted(list(freeze) + order[:U - K - len(freeze)])
    cand = [f for f in frozen if f >= 2 and f not in freeze]
    dynset = set(rng.choice(cand, size=min(dyn, len(cand)), replace=False).tolist()) if dyn else set()
    lines = [f"{U - len(punct) - len(short)} {K} 0 {len(layers)} {len(short)} {len(punct)}", " ".join(layers)]
    if short or punct:
        lines.append(" ".join(str(p) for p in tuple(short) + tuple(punct)))
    for f in frozen:
        if f in dynset:
            a, b = sorted(rng.choice(f, size=2, replace=False).tolist())
            lines.append(f"3 {a} {b} {f}")
        else:
            lines.append(f"1 {f}")
    return "\n".join(lines) + "\n"


def list_metric_gap(metric_bits):
    """The least relative distance between two metrics of one recorded list (inf for one entry)."""
    m = np.sort(np.asarray(metric_bits, np.uint32).view(np.float32).astype(np.float64))
    if len(m) < 2:
        return np.inf
    d = np.diff(m)
    scale = np.maximum(np.maximum(np.abs(m[1:]), np.abs(m[:-1])), 1e-30)
    return float(np.min(d / scale))
