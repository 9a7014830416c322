#!/usr/bin/env python3
"""Rate of genie-aided SC (csrc/polar_genie.hip) on one MI355X: words/s of
PolarListDecoder.genie_run (words generated on the GPU, the genie kernel, the column sums) at
2 dB for three codes: all-Arikan (1024, 512), A^4 x eBCH16 (the trellis innermost) and
A5 x G x A^4 (named layers on the channel side). BCHK_LIB chooses the build, so two builds are
compared by running this once per build, in turn. One JSON line per code, with a checksum of the
counters (the same for every build that decodes the same bits).

  python scripts/bench_polar_genie.py [--words W] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from bchk_pkg import load  # noqa: E402
from polar_lib import arikan_spec  # noqa: E402
from test_polar_mixed import KERNELS, _kernel_text  # noqa: E402
from test_polar_mixed_tiered import any_spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--words", type=int, default=1 << 21)
ap.add_argument("--out", default=None)
a = ap.parse_args()
F = load()
kd = tempfile.mkdtemp()
for name, K in KERNELS.items():
    open(os.path.join(kd, f"{name}.txt"), "w").write(_kernel_text(K))
CASES = [("arikan-1024", arikan_spec(10, 512), None),
         ("A4-bch16", any_spec(("A", "A", "A", "A", "bch16"), 128, 0, (), seed=1), kd),
         ("A5-G-A4", any_spec(("A5", "G", "A", "A", "A", "A"), 120, 0, (), seed=1), kd)]
out = open(a.out, "w") if a.out else None
for tag, spec, kdir in CASES:
    d = F.PolarListDecoder(spec, 1, kernel_dir=kdir)
    d.genie_run(2.0, 1 << 14, seed=1)  # warm-up: layout, buffers
    err, soft, secs = d.genie_run(2.0, a.words, seed=2)
    row = {"code": tag, "U": d.U, "words": a.words, "lib": os.environ.get("BCHK_LIB", "this build"), "seconds": secs,
           "words_s": a.words / secs, "checksum": int(err.sum()) + int(soft.sum() & 0xFFFFFFFF)}
    d.close()
    print(json.dumps(row), flush=True)
    if out:
        out.write(json.dumps(row) + "\n")
        out.flush()
