#!/usr/bin/env python3
"""SC-list over mixed kernels (csrc/polar_mixed.hip) with the reference's extended-BCH kernels:
GPU codewords/s against the C restatement on one core (GPU box). Prints JSON lines.
With arguments (--states, --cases, --reps, --out): the list-state variants against each other,
see compare()."""
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

from bchk_pkg import load  # noqa: E402
from polar_lib import PolarOracle, awgn_llr  # noqa: E402
from test_polar_mixed import KERNELS, _kernel_text, mixed_spec  # noqa: E402

F = load()
kdir = tempfile.mkdtemp()
for name, K in KERNELS.items():
    open(os.path.join(kdir, f"{name}.txt"), "w").write(_kernel_text(K))


def compare(args):
    """--states lds,tiered_mixed[:split],...: decoded codewords/s of each state on each case, by
    device events around `--reps` decode_device calls after a warm-up call, the states taken in
    turn and every row twice; a state that refuses the code gives a line with its message. The raw
    lines go to --out (under profiles/) as well."""
    import torch
    E3, A4E2 = ("bch16",) * 3, ("A",) * 4 + ("bch16",) * 2
    sets = {  # (layers, K, L, batch)
        "parent": [(E3, 2048, 8, 512), (("A",) * 4 + ("bch16",), 128, 8, 8192), (("bch32f",) * 2, 512, 8, 1024),
                   (("bch32f",) * 2, 512, 32, 1024)],
        "past": [(E3, 2048, 16, 512), (A4E2, 2048, 8, 512)],
        "long": [(("A",) + E3, 4096, 8, 256), (("A", "A") + E3, 8192, 4, 256)],
        "splits": [(E3, 2048, 8, 512)],
    }
    out = open(args.out, "a") if args.out else None
    for layers, K, L, B in [c for name in args.cases.split(",") for c in sets[name]]:
        spec = mixed_spec(layers, K, dyn=4, seed=1)
        enc = None
        for rnd in range(2):
            for st in args.states.split(","):
                state, _, split = st.partition(":")
                row = {"layers": "-".join(layers), "K": K, "L": L, "B": B, "state": state, "snr_db": 2.0, "round": rnd}
                try:
                    d = F.PolarListDecoder(spec, L, kernel_dir=kdir, state=state, split=int(split) if split else None)
                except F.BchkError as e:
                    row["refused"] = str(e)
                    print(json.dumps(row), flush=True)
                    continue
                if enc is None:  # the words: the host encoder, AWGN at 2 dB
                    info = np.random.default_rng(2).integers(0, 2, (B, K)).astype(np.uint8)
                    enc = torch.from_numpy(awgn_llr(d.encode(info), 2.0, K / d.N, seed=3)).cuda()
                dev = enc.device
                bufs = (torch.zeros((B, L, K), dtype=torch.uint8, device=dev), torch.zeros((B, L, d.N), dtype=torch.uint8, device=dev),
                        torch.zeros((B, L), dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
                s = torch.cuda.Stream()

                def run():
                    d.decode_device(enc.data_ptr(), B, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                    bufs[3].data_ptr(), stream=s.cuda_stream)
                torch.cuda.synchronize()
                run()
                s.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(args.reps):
                    run()
                e1.record(s)
                s.synchronize()
                ms = e0.elapsed_time(e1) / args.reps
                row.update(d.state_info(), U=d.U, ms_per_call=ms, cw_s=B / (ms * 1e-3),
                           checksum=int(bufs[0].sum().item()) + int(bufs[3].sum().item()))
                d.close()
                print(json.dumps(row), flush=True)
                if out:
                    out.write(json.dumps(row) + "\n")
                    out.flush()


if len(sys.argv) > 1:
    import argparse
    ap = argparse.ArgumentParser(description=compare.__doc__)
    ap.add_argument("--states", default="lds,tiered_mixed")
    ap.add_argument("--cases", default="parent", help="comma list of: parent, past, long, splits")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    compare(ap.parse_args())
    sys.exit(0)
# (layers, K, L, batch, trellis threshold): matrix layers of at least that size take their LLRs
# from the trellis (default 16), smaller ones enumerate the coset
CASES = [(("A",) * 5 + ("bch8",), 128, 8, 4096, 16), (("A",) * 5 + ("bch8",), 128, 8, 4096, 2),
         (("bch8",) + ("A",) * 5, 128, 8, 4096, 16), (("bch8",) + ("A",) * 5, 128, 8, 4096, 2),
         (("A",) * 4 + ("bch16",), 128, 4, 4096, 16), (("A",) * 4 + ("bch16",), 128, 8, 4096, 16),
         (("bch16",) + ("A",) * 4, 128, 8, 4096, 16), (("A",) * 7 + ("bch8",), 512, 8, 1024, 16),
         (("A",) * 3 + ("bch32f",), 128, 4, 1024, 16), (("bch32f",) + ("A",) * 3, 128, 4, 1024, 16)]
for layers, K, L, B, tmin in CASES:
    os.environ["BCHK_POLAR_TRELLIS"] = str(tmin)
    spec = mixed_spec(layers, K, dyn=4, seed=1)
    o = PolarOracle(spec, kdir)
    d = F.PolarListDecoder(spec, L, kernel_dir=kdir)
    info = np.random.default_rng(2).integers(0, 2, (B, K)).astype(np.uint8)
    llr = awgn_llr(o.encode(info), 2.0, K / o.N, seed=3)
    d.decode(llr[:64])
    t0 = time.perf_counter()
    got = d.decode(llr)
    g = time.perf_counter() - t0
    n_cpu = 32 if o.U <= 256 else 8
    t0 = time.perf_counter()
    want = o.decode_batch(llr[:n_cpu], L, threads=1)
    c = time.perf_counter() - t0
    same = all(np.array_equal(a[:n_cpu], b) for a, b in zip(got, want))
    print(json.dumps({"layers": "-".join(layers), "U": o.U, "K": K, "L": L, "B": B, "trellis_min_size": tmin,
                      "gpu_cw_s": B / g,
                      "oracle_cw_s_1core": n_cpu / c, "ratio": (B / g) / (n_cpu / c), "same_as_oracle": same}),
          flush=True)
