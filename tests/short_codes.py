"""The shortened test codes of tests/test_polar_contract.py, by name; oracle/make_golden.py
records three of them with the compiled reference (polar_ref_short_<name>). Only builders: a
specification depends on the kernel matrices, not on where their files lie.

Each is built by polar_lib.shorten: the last s encoder inputs frozen to 0, and s of the symbols
that this makes always 0 shortened. The named code A5 x G x A is the specification of the recorded
fixture named_ref_A5_G_A_short (tests/named_lib.py), which was built the same way.
"""
import os

import numpy as np

import named_lib as NL
from polar_lib import arikan_spec, shorten
from test_polar_mixed import KERNELS, _kernel_text, mixed_spec

# the factor of the large-LLR rows: magnitudes of some 10^4, which a shortened symbol's 100000 must
# still outweigh in every min. With LLRs of order 1 alone no list depends on the mapped value as
# long as it is the largest: a shortened symbol's LLR then only ever wins a g, never a min.
LARGE = np.float32(4096.0)


def write_kernels(d):
    """test_polar_mixed's kernel files, and G / A5 in matrix form for the oracle's encoder."""
    for name, K in dict(KERNELS, G=NL.G, A5=NL.A5).items():
        with open(os.path.join(d, f"{name}.txt"), "w") as f:
            f.write(_kernel_text(K))
    return str(d)


def matrix_form(spec):
    """The specification with G / A5 given as the matrix files of write_kernels()."""
    lines = spec.split("\n")
    lines[1] = " ".join(f"-{n}.txt" if n in ("G", "A5") else n for n in lines[1].split())
    return "\n".join(lines)


def _arikan(n, K, s, punct=(), dyn=0, seed=0):
    return lambda kd: shorten(lambda **kw: arikan_spec(n, K, dyn=dyn, seed=seed, **kw), 1 << n, s, punct)


def _mixed(layers, K, s, punct=(), dyn=0, seed=0):
    U = int(np.prod([2 if n == "A" else len(KERNELS[n]) for n in layers]))
    return lambda kd: shorten(lambda **kw: mixed_spec(layers, K, dyn=dyn, seed=seed, **kw), U, s, punct, kd)


NAMED_FIXTURE = "A5_G_A_short"

SHORT = {
    "arikan_n6": _arikan(6, 24, 5, seed=6),                                # fixture
    "arikan_n7": _arikan(7, 60, 3, punct=(1, 66), dyn=4, seed=7),          # fixture: short + punct + dyn
    "bch8_A_A": _mixed(("bch8", "A", "A"), 14, 2, dyn=2, seed=41),         # enumeration
    "bch16_A": _mixed(("bch16", "A"), 14, 3, dyn=2, seed=42),              # fixture: trellis
    "A_bch16": _mixed(("A", "bch16"), 12, 2, punct=(5,), seed=43),
    "A_bch32f": _mixed(("A", "bch32f"), 28, 3, dyn=2, seed=44),
    "k3_k4_A": _mixed(("k3", "k4", "A"), 10, 2, punct=(7,), dyn=1, seed=45),  # odd sizes
    "A5_G_A": lambda kd: NL.fixture(os.path.join(NL.R.GOLD, f"named_ref_{NAMED_FIXTURE}.txt.gz")).spec,
    "bch64f": _mixed(("bch64f",), 32, 2, seed=19 + 32),                    # test_polar_budget's CODES64[0], shortened
}
FIXTURES = ("arikan_n6", "bch16_A", "arikan_n7")

_specs = {}


def short_spec(name, kernel_dir):
    """The specification text of SHORT[name]; kernel_dir holds write_kernels()'s files."""
    if name not in _specs:
        _specs[name] = SHORT[name](kernel_dir)
    return _specs[name]


def with_large_rows(llr):
    """The upper half of the rows times LARGE."""
    out = np.array(llr, np.float32)
    out[len(out) // 2:] *= LARGE
    assert 1000.0 < np.abs(out).max() < 100000.0
    return out
