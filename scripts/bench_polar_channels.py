#!/usr/bin/env python3
"""Rate of the polar channel front-end (polar_gen_kernel, csrc/polar_channel.hip) on one MI355X:
words/s of generate_device on the all-Arikan (1024, 512) code at a batch of 2^16 words (the batch
of DESIGN.md 5.13), for AWGN through bchk_polar_generate_device and, where the library has them,
for AWGN, Rayleigh and the BSC through bchk_polar_generate_channel_device and for block (S = 16),
correlated (rho = 0.9) and Rician (K = 3) fading through bchk_polar_generate_fading_device.
--log2n chooses another length 2^n at rate 1/2 (DESIGN.md 5.5 "Fading models": n = 10 at a batch
of 16384, n = 14 at 2048). The library is bound
here with ctypes, only the calls used, so that BCHK_LIB may name a build from before the channel
entry points: two builds are compared by running this once per build, in turn, in one session.
Device events around `reps` launches, best and median of `rounds` after a warm-up. One JSON line
per row, with a checksum of the LLR bits (the same for every build that generates the same words).

  python scripts/bench_polar_channels.py [--log2n n] [--batch B] [--reps R] [--rounds N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from polar_lib import arikan_spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=10)
ap.add_argument("--batch", type=int, default=1 << 16)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()

path = os.environ.get("BCHK_LIB") or os.path.join(REPO, "polar-codes-with-bch-kernel_amd", "lib", "libbchk.so")
L = C.CDLL(path)
vp, sz, i32, u64, dbl = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_double
L.bchk_polar_create.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
L.bchk_polar_destroy.argtypes = [vp]
L.bchk_polar_destroy.restype = None
L.bchk_polar_generate_device.argtypes = [vp, dbl, sz, u64, u64, vp, vp, vp, vp]
L.bchk_last_error.restype = C.c_char_p
rows = [("awgn", "bchk_polar_generate_device", None, 2.0)]
if hasattr(L, "bchk_polar_generate_channel_device"):
    L.bchk_polar_generate_channel_device.argtypes = [vp, i32, dbl, sz, u64, u64, vp, vp, vp, vp, vp, vp]
    rows += [("awgn", "bchk_polar_generate_channel_device", 0, 2.0), ("rayleigh", "bchk_polar_generate_channel_device", 1, 2.0),
             ("bsc", "bchk_polar_generate_channel_device", 2, 0.05)]
if hasattr(L, "bchk_polar_generate_fading_device"):  # (kind, its parameter) in place of the channel
    L.bchk_polar_generate_fading_device.argtypes = [vp, i32, dbl, dbl, sz, u64, u64, vp, vp, vp, vp, vp, vp]
    rows += [("block S=16", "bchk_polar_generate_fading_device", (0, 16.0), 2.0),
             ("correlated rho=0.9", "bchk_polar_generate_fading_device", (1, 0.9), 2.0),
             ("rician K=3", "bchk_polar_generate_fading_device", (2, 3.0), 2.0)]

h = vp()
N, K, B = 1 << a.log2n, 1 << (a.log2n - 1), a.batch
if L.bchk_polar_create(arikan_spec(a.log2n, K).encode(), 1, 0, C.byref(h)):
    sys.exit(L.bchk_last_error().decode())
stream = torch.cuda.Stream()
info = torch.zeros((B, K), dtype=torch.uint8, device="cuda")
cw = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
llr = torch.zeros((B, N), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
out = open(a.out, "a") if a.out else None
for tag, entry, channel, param in rows:
    def call():
        if channel is None:
            rc = L.bchk_polar_generate_device(h, param, B, 1, 0, info.data_ptr(), cw.data_ptr(), llr.data_ptr(),
                                              stream.cuda_stream)
        elif isinstance(channel, tuple):
            rc = L.bchk_polar_generate_fading_device(h, channel[0], channel[1], param, B, 1, 0, info.data_ptr(),
                                                     cw.data_ptr(), llr.data_ptr(), None, None, stream.cuda_stream)
        else:
            rc = L.bchk_polar_generate_channel_device(h, channel, param, B, 1, 0, info.data_ptr(), cw.data_ptr(),
                                                      llr.data_ptr(), None, None, stream.cuda_stream)
        if rc:
            sys.exit(L.bchk_last_error().decode())
    ms = []
    with torch.cuda.stream(stream):
        for rnd in range(a.rounds + 1):  # round 0 warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                call()
            e1.record(stream)
            e1.synchronize()
            if rnd:
                ms.append(e0.elapsed_time(e1) / a.reps)
    row = {"channel": tag, "entry": entry, "lib": os.environ.get("BCHK_LIB", "this build"), "batch": B, "N": N,
           "us_per_word_median": statistics.median(ms) * 1e3 / B,
           "ms_best": min(ms), "ms_median": statistics.median(ms), "ms_max": max(ms), "words_s_best": B / min(ms) * 1e3,
           "checksum": int(llr.view(torch.int32).to(torch.int64).sum().item()) & 0xFFFFFFFF}
    print(json.dumps(row), flush=True)
    if out:
        out.write(json.dumps(row) + "\n")
        out.flush()
L.bchk_polar_destroy(h)
