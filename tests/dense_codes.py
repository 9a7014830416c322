"""Codes with DENSE dynamic freezing: more than 32 constraints live at once, so the upper half of
the decoders' 64-bit dynamic-freezing mask (PathRegs::dm, csrc/polar_list_device.h) carries
values, and constraints of 65 and of 130 terms, which take the device encoder's term loop
(csrc/polar_enc_device.h) through a second and a third pass. Built by polar_lib.dense_arikan_spec
and test_polar_mixed.dense_mixed_spec; the names say how many constraints are live at once.

FIXTURES are recorded from the compiled vendored library (oracle/make_golden.py polar,
tests/golden/polar_ref_dyn_*); the others have the C oracle as their reference.
Shared by the generator, tests/test_polar_reference.py, tests/test_polar_dense_spec.py and
tests/test_polar_dense_dyn.py.
"""
from polar_lib import dense_arikan_spec
from test_polar_mixed import dense_mixed_spec

WIDE = (65, 130)  # terms before the frozen symbol: one pass of 64 lanes plus one lane; three passes

ARIKAN = {
    # (256, 64): 64 constraints live across symbol 128, mask bits 0..63
    "dyn_arikan_n8_a64": dict(n=8, K=64, active=64, pivot=128, lo_info=24, seed=8),
    # (128, 32): 33 live across symbol 64 (bit 32 alone in the high word), three more on reused bits
    "dyn_arikan_n7_a33": dict(n=7, K=32, active=33, pivot=64, lo_info=8, late=3, seed=7),
    # (512, 300): K large enough for the wide constraints over Arikan layers; not recorded
    "dyn_arikan_n9_a64": dict(n=9, K=300, active=64, pivot=256, lo_info=150, widths=WIDE, late=4, seed=9),
}
MIXED = {
    # U = 256 over the 16 x 16 and 8 x 8 extended-BCH kernels: 40 live across symbol 160, two late
    "dyn_A_bch16_bch8_a40": dict(layers=("A", "bch16", "bch8"), K=176, active=40, pivot=160, lo_info=136,
                                 widths=WIDE, late=2, seed=16),
    # U = 64, for the budgeted path (every 8 x 8 layer through the search): 34 live; not recorded
    "dyn_bch8_A_A_A_a34": dict(layers=("bch8", "A", "A", "A"), K=18, active=34, pivot=16, lo_info=8, late=2, seed=5),
}
FIXTURES = ("dyn_arikan_n8_a64", "dyn_arikan_n7_a33", "dyn_A_bch16_bch8_a40")
SNR = {"dyn_arikan_n8_a64": 1.0, "dyn_arikan_n7_a33": 1.0, "dyn_A_bch16_bch8_a40": 2.0}  # Eb/N0 of the recorded rows
# one more than the mask holds, otherwise dyn_arikan_n8_a64
OVER = dict(n=8, K=64, active=65, pivot=128, lo_info=24, seed=8)


def spec(name):
    return dense_arikan_spec(**ARIKAN[name]) if name in ARIKAN else dense_mixed_spec(**MIXED[name])


def layers(name):
    return ("A",) * ARIKAN[name]["n"] if name in ARIKAN else MIXED[name]["layers"]


def claimed_active(name):
    return int(name.rsplit("_a", 1)[1])
