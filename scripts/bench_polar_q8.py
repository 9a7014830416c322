#!/usr/bin/env python3
"""Decode throughput of the int8 SC-list decoder (csrc/polar_sclist_q8.hip) against the f32
decoders on one MI355X, on the same device buffers.

Per shape (n, K, L, the f32 state it is compared with): B words of bchk_polar_generate_device's
stream at --snr, quantised once by bchk_polar_quantize_device (--scale, --qmax). A sample =
--steps decode calls over the B resident rows, timed with HIP events on the decoder's stream;
after a warm-up sample of each decoder, --repeats samples are taken alternating f32 and q8. One
JSON line per shape: median codewords/s of both with their min and max, the ratio of the medians,
LDS bytes and waves per CU of both contexts, and the block error rate of the best path of both
(the same words), so that a speed is never read without what it decodes.

    python scripts/bench_polar_q8.py

--state tiered_q8 measures the tiered int8 decoder (csrc/polar_sclist_q8_tiered.hip)
instead: per shape the decoders that exist for it -- tiered f32, LDS q8 where the code fits, tiered
q8 -- alternate in one run, sampled the same way, and the line carries each one's figures, the
ratio of tiered q8 to each of the others, and the workspace bytes.

    python scripts/bench_polar_q8.py --state tiered_q8
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = ((10, 512, 8, "lds", 1 << 15), (10, 512, 32, "lds", 1 << 14), (11, 1024, 32, "tiered", 1 << 13))
# --state tiered_q8: (n, K, L, the LDS q8 decoder takes it, B)
TIERED_SHAPES = ((10, 512, 8, True, 1 << 15), (10, 512, 32, True, 1 << 14), (11, 1024, 32, True, 1 << 13),
                 (12, 2048, 32, False, 1 << 12), (14, 8192, 8, False, 1 << 12), (14, 8192, 32, False, 1 << 11))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--scale", type=float, default=4.0)
    ap.add_argument("--qmax", type=int, default=63)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--state", choices=("lds", "tiered_q8"), default="lds",
                    help="the q8 decoder measured: the LDS one against f32, or the tiered one against tiered f32 and LDS q8")
    ap.add_argument("--shapes", type=int, nargs="*", help="indices into the table of shapes (default: all)")
    a = ap.parse_args()

    import torch
    from bchk_pkg import load
    from polar_lib import arikan_spec

    F = load()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiered = a.state == "tiered_q8"
    table = TIERED_SHAPES if tiered else SHAPES
    for n, K, L, state, B in (table if a.shapes is None else [table[i] for i in a.shapes]):
        spec = arikan_spec(n, K, seed=1)
        if tiered:
            dec = {"tiered_f32": F.PolarListDecoder(spec, L, state="tiered")}
            if state:
                dec["lds_q8"] = F.PolarListDecoder(spec, L, llr="q8")
            dec["q8"] = F.PolarListDecoder(spec, L, llr="q8", state="tiered_q8")
        else:
            dec = {"f32": F.PolarListDecoder(spec, L, state=state), "q8": F.PolarListDecoder(spec, L, llr="q8")}
        N = dec["q8"].N
        t_tx = torch.zeros((B, K), dtype=torch.uint8, device=dev)
        t_llr = torch.zeros((B, N), dtype=torch.float32, device=dev)
        t_q = torch.zeros((B, N), dtype=torch.int8, device=dev)
        t_info = torch.zeros((B, L, K), dtype=torch.uint8, device=dev)
        t_cw = torch.zeros((B, L, N), dtype=torch.uint8, device=dev)
        t_met = torch.zeros((B, L), dtype=torch.float32, device=dev)
        t_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        dec["q8"].generate_device(a.snr, B, t_llr.data_ptr(), t_tx.data_ptr(), seed=1)
        dec["q8"].quantize_device(t_llr.data_ptr(), B * N, t_q.data_ptr(), a.scale, a.qmax)
        dec["q8"].sync()
        src = {kind: t_q if d.llr == "q8" else t_llr for kind, d in dec.items()}

        def sample(kind):
            d = dec[kind]
            st = torch.cuda.ExternalStream(d.stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.steps):
                d.decode_device(src[kind].data_ptr(), B, t_info.data_ptr(), t_cw.data_ptr(), t_met.data_ptr(),
                                t_cnt.data_ptr())
            e1.record(st)
            d.sync()
            return B * a.steps / (e0.elapsed_time(e1) * 1e-3)

        fer, rates = {}, {kind: [] for kind in dec}
        for kind in rates:  # warm-up, and what each decoder makes of these words
            sample(kind)
            fer[kind] = float((t_info[:, 0] != t_tx).any(dim=1).float().mean())
        for _ in range(a.repeats):
            for kind in rates:
                rates[kind].append(sample(kind))
        row = {"metric": "SC-list decode codewords/s, q8 against f32", "unit": "codewords/s",
               "config": {"workload": f"Arikan polar ({N},{K}), L={L}, Eb/N0={a.snr} dB", "batch": B, "steps": a.steps,
                          "repeats": a.repeats, "scale": a.scale, "qmax": a.qmax,
                          "f32_state": "tiered" if tiered else state}}
        if tiered:
            row["metric"] = "SC-list decode codewords/s, tiered q8 against tiered f32 and LDS q8"
        for kind, d in dec.items():
            si = d.state_info()
            row[kind] = {"median": statistics.median(rates[kind]), "min": min(rates[kind]), "max": max(rates[kind]),
                         "lds_bytes": si["lds_bytes"], "split": si["split"], "waves_per_cu": si["grid"] / cus,
                         "fer_best_path": fer[kind]}
            if tiered:
                row[kind]["workspace_bytes"] = si["workspace_bytes"]
        for kind in dec:
            if kind != "q8":
                row[f"q8_over_{kind}"] = row["q8"]["median"] / row[kind]["median"]
        print(json.dumps(row), flush=True)
        for d in dec.values():
            d.close()


if __name__ == "__main__":
    main()
