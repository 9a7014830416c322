#!/usr/bin/env python3
"""Throughput of the GPU SC-list decoder (csrc/polar_sclist.hip) on one MI355X.

A step = one bchk_polar_decode_device call over B resident codewords' LLRs (float32) of an
Arikan polar code (PW frozen set, optional dynamic constraints), AWGN at --snr. Timed with
HIP events on the decoder's own stream. Prints one JSON line: codewords/s, the kernel's
average duration, the algorithmic HBM bytes per codeword (4N LLR read + L(K + N) bytes of
information/codeword rows + 4L metrics + 4 count written) against the 8 TB/s roof, FER of
the best path, and the oracle (oracle/polar_oracle.c, one host core) on a bounded sample.

    python scripts/bench_polar.py --n 10 --K 512 --L 8 --snr 2.0 --batch 65536

--state tiered [--split S] decodes with the tiered state (csrc/polar_sclist_tiered.hip; codes past
the LDS limit need it); --grids G makes the batch G times the context's persistent grid, so every
wave decodes the same number of codewords. The line then also carries the split in use, LDS and
workspace bytes per codeword in flight, the grid and the waves per CU.

    python scripts/bench_polar.py --n 12 --K 2048 --L 32 --state tiered --grids 8

--sim times the whole simulation instead (bchk_polar_sweep_device: words generated, decoded and
counted on the GPU, one Eb/N0 point cut by words) in words/s of wall time, at (1024, 512) and
(64, 32) with L = 8, beside the decode-only rate of the same context in the same run (device
events around bchk_polar_decode_device over LLRs from bchk_polar_generate_device). One JSON
line per shape.

    python scripts/bench_polar.py --sim --snr 2.0
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0


SIM_SHAPES = ((10, 512, 8), (6, 32, 8))  # n, K, L


def sim(a):
    import torch
    from bchk_pkg import load
    from polar_lib import arikan_spec

    dev = torch.device("cuda:0")
    for n, K, L in SIM_SHAPES:
        d = load().PolarListDecoder(arikan_spec(n, K, dyn=a.dyn, seed=1), L)
        N = d.N
        B = a.sim_batch or (1 << 14 if n >= 10 else 1 << 18)
        t_llr = torch.zeros((B, N), dtype=torch.float32, device=dev)
        t_info = torch.zeros((B, L, K), dtype=torch.uint8, device=dev)
        t_cw = torch.zeros((B, L, N), dtype=torch.uint8, device=dev)
        t_met = torch.zeros((B, L), dtype=torch.float32, device=dev)
        t_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        d.generate_device(a.snr, B, t_llr.data_ptr(), seed=1)
        st = torch.cuda.ExternalStream(d.stream)

        def run():
            d.decode_device(t_llr.data_ptr(), B, t_info.data_ptr(), t_cw.data_ptr(), t_met.data_ptr(),
                            t_cnt.data_ptr())

        for _ in range(a.warmup):
            run()
        d.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.steps):
            run()
        e1.record(st)
        d.sync()
        decode_cps = B * a.steps / (e0.elapsed_time(e1) * 1e-3)
        # the sweep: the same words (stream 1 from word 0), `steps` batches, never cut by errors
        words = B * a.steps
        d.sweep_device(a.snr, 0.0, 1, B, 1 << 62, seed=1, batch=B)  # warm-up: buffers, code objects
        recs, secs, done = d.sweep_device(a.snr, 0.0, 1, words, 1 << 62, seed=1, batch=B)
        c = recs[0][1]
        assert done == words and c[0] == words
        print(json.dumps({
            "metric": "polar simulation words/s", "value": done / secs, "unit": "words/s",
            "config": {"workload": f"Arikan polar ({N},{K}) dyn={a.dyn}, L={L}, Eb/N0={a.snr} dB", "batch": B,
                       "words": words},
            "sweep_seconds": secs, "decode_only_codewords_per_s": decode_cps,
            "sweep_over_decode_only": (done / secs) / decode_cps,
            "counters": dict(zip(load().POLAR_COUNTERS, c)), "fer": c[1] / c[0]}), flush=True)
        d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sim", action="store_true", help="time sweep_device end to end at the two standard shapes")
    ap.add_argument("--sim-batch", type=int, default=0, help="words per batch of --sim (0: 2^14 / 2^18)")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--K", type=int, default=512)
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--dyn", type=int, default=0)
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cw", action="store_true", help="do not write the codeword rows")
    ap.add_argument("--cpu-seconds", type=float, default=5.0)
    ap.add_argument("--state", choices=("lds", "tiered"), default="lds")
    ap.add_argument("--split", type=int, default=None, help="tiered: the boundary (default: the library's choice)")
    ap.add_argument("--grids", type=int, default=0, help="batch = this many times the persistent grid")
    a = ap.parse_args()
    if a.sim:
        return sim(a)

    import torch
    from bchk_pkg import load
    from polar_lib import PolarOracle, arikan_spec, awgn_llr

    spec = arikan_spec(a.n, a.K, dyn=a.dyn, seed=1)
    o = PolarOracle(spec) if a.n <= 12 else None  # the C oracle stops at U = 4096
    d = load().PolarListDecoder(spec, a.L, state=a.state, split=a.split)
    si = d.state_info()
    N, K, L, B = d.N, d.K, d.L, a.grids * si["grid"] if a.grids else a.batch
    rng = np.random.default_rng(1)
    base = min(B, max(64, (1 << 24) >> a.n))  # distinct words (host-encoded), tiled over the batch
    info = rng.integers(0, 2, (base, K)).astype(np.uint8)
    llr = awgn_llr(d.encode(info), a.snr, K / N, seed=2)
    reps = (B + base - 1) // base
    dev = torch.device("cuda:0")
    t_llr = torch.from_numpy(np.tile(llr, (reps, 1))[:B]).to(dev)
    t_info = torch.zeros((B, L, K), dtype=torch.uint8, device=dev)
    t_cw = None if a.no_cw else torch.zeros((B, L, N), dtype=torch.uint8, device=dev)
    t_met = torch.zeros((B, L), dtype=torch.float32, device=dev)
    t_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.ExternalStream(d.stream)

    def run():
        d.decode_device(t_llr.data_ptr(), B, t_info.data_ptr(),
                        0 if t_cw is None else t_cw.data_ptr(), t_met.data_ptr(),
                        t_cnt.data_ptr())

    for _ in range(a.warmup):
        run()
    d.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(st)
    for _ in range(a.steps):
        run()
    e1.record(st)
    d.sync()
    wall = time.perf_counter() - t0
    ms = e0.elapsed_time(e1) / a.steps
    cps = B / (ms * 1e-3)
    fer = float((t_info[:base, 0].cpu().numpy() != info).any(axis=1).mean())
    algo = 4 * N + L * (K + (0 if a.no_cw else N)) + 4 * L + 4
    gbs = algo * B / (ms * 1e-3) / 1e9

    # parity spot check + CPU baseline on a bounded sample (oracle, one core)
    cpu = None
    if a.cpu_seconds > 0 and o is not None:
        t = time.perf_counter()
        done = 0
        want = []
        while time.perf_counter() - t < a.cpu_seconds and done < base:
            want.append(o.decode(llr[done], L))
            done += 1
        cpu_s = time.perf_counter() - t
        cpu = {"value": done / cpu_s, "unit": "codewords/s", "cores": 1, "kind": "port",
               "sample": f"{done} codewords of the same batch, oracle/polar_oracle.c"}
        got_i = t_info[:done].cpu().numpy()
        got_m = t_met[:done].cpu().numpy()
        for b, (c, wi, wc, wm) in enumerate(want):
            assert np.array_equal(got_i[b, :c], wi[:c]), f"info mismatch row {b}"
            assert np.array_equal(got_m[b, :c].view(np.uint32), wm[:c].view(np.uint32))
    print(json.dumps({
        "metric": "SC-list codewords/s", "value": cps, "unit": "codewords/s",
        "config": {"workload": f"Arikan polar ({N},{K}) dyn={a.dyn}, L={L}, Eb/N0={a.snr} dB",
                   "batch": B, "write_codewords": not a.no_cw, "state": a.state},
        "state": dict(si, waves_per_cu=si["grid"] / torch.cuda.get_device_properties(0).multi_processor_count),
        "ms_per_step": ms, "wall_s": wall, "fer_best_path": fer,
        "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": gbs / HBM_PEAK_GBS, "algo_bytes_per_codeword": algo},
        "cpu_baseline": cpu}))


if __name__ == "__main__":
    main()
