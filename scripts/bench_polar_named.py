#!/usr/bin/env python3
"""SC-list decoding of the (96, 48) code A A A A A G of tests/golden/named_ref_A_A_A_A_A_G at
L = 8: the named form (G through its f/g processor) or the matrix form of the same code (G as
the kernel file -G.txt, coset enumeration). One form per process (BCHK_LIB chooses the build);
a shell loop alternates them. Words come from the on-GPU channel at 2 dB; the timed call is
decode_device between two synchronisations. Prints one JSON line, and a checksum of the lists
so that the two forms can be compared (G is the innermost layer: the lists are the same).

  python scripts/bench_polar_named.py named|matrix [words] [repeats]
"""
import json
import os
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import named_lib as NL  # noqa: E402
import polar_ref_lib as R  # noqa: E402
from bchk_pkg import load  # noqa: E402

form = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 17
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
L = 8
spec = NL.fixture(os.path.join(R.GOLD, "named_ref_A_A_A_A_A_G.txt.gz")).spec
kdir = tempfile.mkdtemp()
if form == "matrix":
    lines = spec.split("\n")
    lines[1] = " ".join("-G.txt" if n == "G" else n for n in lines[1].split())
    spec = "\n".join(lines)
    open(os.path.join(kdir, "G.txt"), "w").write(R.kernel_text(NL.G))
d = load().PolarListDecoder(spec, L, kernel_dir=kdir)
dev = "cuda:0"
llr = torch.zeros((B, d.N), dtype=torch.float32, device=dev)
info = torch.zeros((B, L, d.K), dtype=torch.uint8, device=dev)
cw = torch.zeros((B, L, d.N), dtype=torch.uint8, device=dev)
met = torch.zeros((B, L), dtype=torch.float32, device=dev)
cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
torch.cuda.synchronize()
d.generate_device(2.0, B, llr.data_ptr(), seed=1)
d.sync()


def once():
    t0 = time.perf_counter()
    d.decode_device(llr.data_ptr(), B, info.data_ptr(), cw.data_ptr(), met.data_ptr(), cnt.data_ptr())
    d.sync()
    return time.perf_counter() - t0


for _ in range(3):
    once()
ts = sorted(once() for _ in range(reps))
crc = 0
for t in (info, cnt):  # (the two forms sum their metrics differently)
    crc = zlib.crc32(t.cpu().numpy().tobytes(), crc)
print(json.dumps({"form": form, "lib": os.environ.get("BCHK_LIB", "this build"), "words": B, "L": L, "repeats": reps,
                  "ms_median": 1e3 * float(np.median(ts)), "ms_min": 1e3 * ts[0], "ms_max": 1e3 * ts[-1],
                  "words_per_s_median": B / float(np.median(ts)), "lists_crc32": f"{crc:08x}"}), flush=True)
