"""Timings of the bit-reversible sampler on the graph-replayed engine (FFHQ-size UNet, random weights):

  eval     ms per step of ReversibleEngine (the "sample" schedule from noise, 50 steps) against the plain DenoiseEngine's "ddim"
           step at the same batch - its path is untouched by the reversible sampler and so stands for the parent commit - bf16,
           batch 1 / 8 / 64: ALTERNATED pairs on one box, each run ended by a device synchronise; the median and the range of the
           pair deltas.
  kernel   afldm_rev_step alone as ONE graph of 20 launches at batch 1 and 64 (device events around `--replays` replays), next to
           afldm_ddim_step captured the same way.  The update moves about 38 bytes per element (int64 far and near read and
           written, fp32 lat written, bf16 eps read) against afldm_ddim_step's 10.
  drift    for the record only: the rel-RMS between the reversible sampler's and plain DDIM's final latents at N = 50 from the
           same noise, with these seeded random weights.  It says nothing about a trained model.

One JSON line per measurement.  `python tools/bench_rev.py [--what eval,kernel,drift] [--reps 5] [--dtype bf16]`."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sde import ffhq_unet  # noqa: E402

STEPS = 50


def bench_eval(a, unet):
    from afldm_amd.engine import DenoiseEngine, ReversibleEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    s = unet.config.sample_size
    for batch in (1, 8, 64):
        x = torch.randn(batch, 4, s, s, generator=torch.Generator().manual_seed(0))
        sch = ffhq_ddim_scheduler()
        plain = DenoiseEngine(unet, sch.schedule(STEPS), batch, STEPS)
        rev = ReversibleEngine(unet, sch.reversible_schedule(STEPS, "sample", False), batch, STEPS)
        runs = {"plain": lambda: plain.run(x), "rev": lambda: rev.run(x)}
        times = {k: [] for k in runs}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / STEPS * 1e3)
        p, r = statistics.median(times["plain"]), statistics.median(times["rev"])
        deltas = [(u - v) * 1e3 for u, v in zip(times["rev"], times["plain"])]
        print(json.dumps({"what": "eval", "batch": batch, "dtype": a.dtype, "steps": STEPS, "plain_ms": round(p, 4), "rev_ms": round(r, 4),
                          "median_pair_delta_us": round(statistics.median(deltas), 2),
                          "pair_deltas_us": [round(d, 2) for d in deltas], "plain_runs_ms": [round(t, 4) for t in times["plain"]],
                          "rev_runs_ms": [round(t, 4) for t in times["rev"]]}), flush=True)
        del plain, rev


def bench_kernel(a, dtype):
    from afldm_amd import ops
    C, S, L = 4, 32, 20
    for batch in (1, 64):
        g = torch.Generator().manual_seed(0)
        far = torch.randint(-2 ** 33, 2 ** 33, (batch, C, S, S), generator=g, dtype=torch.int64).cuda()
        near = torch.randint(-2 ** 33, 2 ** 33, (batch, C, S, S), generator=g, dtype=torch.int64).cuda()
        x = torch.randn(batch, C, S, S, generator=g).cuda()
        eps = (0.1 * torch.randn(batch, S, S, C, generator=g)).to("cuda", dtype)
        bad = torch.zeros(batch, dtype=torch.int32, device="cuda")
        lat = torch.empty(batch, C, S, S, device="cuda")
        idx = torch.zeros(1, dtype=torch.int32, device="cuda")
        # rows under which thousands of launches on the same buffers only drift linearly, and stay in range
        rcoef = torch.tensor([[0.0, 1e-4, 1.0, 0.0]], dtype=torch.float32).cuda().reshape(-1)
        dcoef = torch.tensor([[1.0, 0.4, 1.0, 0.39]], dtype=torch.float32).cuda().reshape(-1)
        calls = {"rev": lambda: ops.rev_step(far, near, eps, bad, rcoef, idx, out=lat),
                 "ddim": lambda: ops.ddim_step(x, eps, dcoef, idx, out=x)}
        for name, fn in calls.items():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(L):
                    fn()
            for _ in range(5):
                graph.replay()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.replays):
                    graph.replay()
                t1.record()
                t1.synchronize()
                ts.append(t0.elapsed_time(t1) * 1e3 / a.replays)
            us = statistics.median(ts)
            per = {"rev": 8 * 4 + 4 + eps.element_size(), "ddim": 4 * 2 + eps.element_size()}[name]
            print(json.dumps({"what": "kernel", "kernel": name, "batch": batch, "dtype": a.dtype, "launches_per_graph": L,
                              "graph_us": round(us, 3), "us_per_launch": round(us / L, 3), "runs_graph_us": [round(t, 3) for t in ts],
                              "bytes_per_element": per, "flagged": int(bad.sum())}), flush=True)


def bench_drift(a, unet):
    from afldm_amd.engine import DenoiseEngine, ReversibleEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    s = unet.config.sample_size
    x = torch.randn(8, 4, s, s, generator=torch.Generator().manual_seed(0))
    sch = ffhq_ddim_scheduler()
    plain = DenoiseEngine(unet, sch.schedule(STEPS), 8, STEPS).run(x).double()
    rev = ReversibleEngine(unet, sch.reversible_schedule(STEPS, "sample", False), 8, STEPS).run(x).latents().double()
    rel = float((rev - plain).pow(2).mean().sqrt() / plain.pow(2).mean().sqrt())
    print(json.dumps({"what": "drift", "batch": 8, "dtype": a.dtype, "steps": STEPS, "rel_rms_rev_vs_ddim": round(rel, 5),
                      "note": "seeded random weights: says nothing about a trained model"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--what", default="eval,kernel,drift")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    if not torch.cuda.is_available():
        raise SystemExit("bench_rev needs an MI355X: there is no CPU path")
    what = a.what.split(",")
    if "kernel" in what:
        bench_kernel(a, dtype)
    if "eval" in what or "drift" in what:
        unet = ffhq_unet(dtype)
        if "eval" in what:
            bench_eval(a, unet)
        if "drift" in what:
            bench_drift(a, unet)


if __name__ == "__main__":
    main()
