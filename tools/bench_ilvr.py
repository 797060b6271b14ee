"""ILVR reference-guided sampling on the graph-replayed engine: wall time against its eager loop, and the update kernel against
what it replaces (FFHQ-size UNet, random weights).

Default: MyLDMPipeline.ilvr_latents, 50 steps, down factor 4, eta 1, at batch 1 and batch 16 with a CPU generator.  Each batch
runs once to warm up (capture, packing, workspaces); then graph and eager runs ALTERNATE `--reps` times, each ended by a device
synchronise, and the medians are printed: one JSON line per batch size.

`--kernel-only`: no UNet.  At B = 16 and 64 (C = 4, S = 32, bf16 eps) three loops of `--launches` updates each are captured into
one graph apiece and replayed `--reps` times between device events: afldm_ilvr_step on w = 1 rows, on w = 0 rows, afldm_sde_step,
and the unfused composition the ILVR kernel replaces (sde_step, subtract, to_nhwc, af_resample, to_nchw, add).  Prints the median
time per update in microseconds - replay time over launches, so the gaps between the launches of a graph are in it - and is the
workload for a `rocprofv3 --kernel-trace --stats` run of its own.

Every GPU step (a batch size, or the kernel loops) runs in a child process of its own under a time limit (`--limit` seconds);
after a step that fails or runs out of time nothing more is started.
`python tools/bench_ilvr.py [--dtype bf16] [--reps 3] [--batches 1,16] [--kernel-only]`"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall(a, batch):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from tools.bench_sde import ffhq_unet
    unet = ffhq_unet(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    s = unet.config.sample_size
    g = torch.Generator().manual_seed(0)
    x = torch.randn(batch, 4, s, s, generator=g)
    ref = 0.8 * torch.randn(batch, 4, s, s, generator=g)

    def run(use_graph):
        out = pipe.ilvr_latents(ref, down_factor=a.down_factor, num_inference_steps=a.steps, eta=a.eta, latents=x,
                                generator=torch.Generator().manual_seed(1), use_graph=use_graph)
        torch.cuda.synchronize()
        return out
    run(True), run(False)                                             # warm-up of both
    tg, te = [], []
    for _ in range(a.reps):
        for use_graph, ts in ((True, tg), (False, te)):
            t0 = time.perf_counter()
            run(use_graph)
            ts.append(time.perf_counter() - t0)
    gm, em = statistics.median(tg), statistics.median(te)
    print(json.dumps({"what": "ilvr", "dtype": a.dtype, "batch": batch, "steps": a.steps, "eta": a.eta, "down_factor": a.down_factor,
                      "graph_s": round(gm, 4), "eager_s": round(em, 4), "graph_ms_per_step": round(gm / a.steps * 1e3, 3),
                      "eager_ms_per_step": round(em / a.steps * 1e3, 3), "speedup": round(em / gm, 2),
                      "graph_runs_s": [round(t, 4) for t in tg], "eager_runs_s": [round(t, 4) for t in te]}), flush=True)


def kernels(a):
    from afldm_amd import ops
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    C, S, n = 4, 32, a.launches
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    L = ilvr_filter(S, a.down_factor).float().cuda()
    row = (1.0, -0.5, -float("inf"), float("inf"), 0.83, 0.28, 0.49, 0.83, 0.56)          # |a p| < 1: chained updates stay finite
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    for B in (16, 64):
        g = torch.Generator("cuda").manual_seed(B)
        x = torch.randn(B, C, S, S, device="cuda", generator=g)
        ref = torch.randn(B, C, S, S, device="cuda", generator=g)
        eps = torch.randn(B, S, S, C, device="cuda", generator=g).to(dtype)
        noise2 = torch.randn(1, 2, B, C, S, S, device="cuda", generator=g)
        noise1 = noise2[:, 1]
        coef = {w: torch.tensor(row + (w, 0.0, 0.0), dtype=torch.float32, device="cuda") for w in (1.0, 0.0)}
        sde = torch.tensor(row[:4] + (0.0,) + row[4:7], dtype=torch.float32, device="cuda")      # (p, q, lo, hi, 0, a, b, c)
        d_nhwc, work = torch.empty(B, S, S, C, dtype=dtype, device="cuda"), torch.empty(B * S * S * C, device="cuda")
        lat = x.clone()

        def unfused():
            xp = ops.sde_step(lat, eps, noise1, sde, zero)
            d = torch.sub(ref, xp)
            low = ops.to_nchw(ops.af_resample(ops.to_nhwc(d, dtype, out=d_nhwc), L, workspace=work))
            torch.add(xp, low, out=lat)
        loops = {"ilvr_step_w1": lambda: ops.ilvr_step(lat, eps, ref, noise2, L, L, coef[1.0], zero, out=lat),
                 "ilvr_step_w0": lambda: ops.ilvr_step(lat, eps, ref, noise2, L, L, coef[0.0], zero, out=lat),
                 "sde_step": lambda: ops.sde_step(lat, eps, noise1, sde, zero, out=lat),
                 "unfused_six_launches": unfused}
        res = {}
        for name, fn in loops.items():
            lat.copy_(x)
            fn()                                                          # warm-up outside the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(n):
                    fn()
            ts = []
            for _ in range(a.reps + 1):
                lat.copy_(x)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                graph.replay()
                t1.record()
                torch.cuda.synchronize()
                ts.append(t0.elapsed_time(t1) * 1e3 / n)
            res[name + "_us"] = round(statistics.median(ts[1:]), 2)
        print(json.dumps(dict({"kernel_only": True, "dtype": a.dtype, "batch": B, "C": C, "S": S, "launches_per_replay": n}, **res)),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--eta", type=float, default=1.0)
    ap.add_argument("--down-factor", type=int, default=4)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "kernels":
        return kernels(a)
    if a.child is not None:
        return wall(a, int(a.child))
    # one child process per GPU step, each under its own time limit; nothing is started after one that fails
    for step in (["kernels"] if a.kernel_only else a.batches.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step] + [v for v in sys.argv[1:] if v != "--kernel-only"]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps({"what": "ilvr", "step": step, "failed": rc}), flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
