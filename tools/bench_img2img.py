"""Timings of image-to-image sampling (SDEdit with a change map) on the graph-replayed engine (FFHQ-size UNet, random weights, eta = 0):

  kernel   afldm_sdedit_step alone against afldm_repaint_step at the same shape [B, 4, 32, 32], bf16 eps, batch 1 / 8 / 64: device
           events around `--launches` back-to-back launches, the two kernels ALTERNATED `--reps` times, medians; with the bytes each
           moves per element and the HBM fraction that makes (peak from --hbm-tbs).  Back-to-back launches of a microsecond kernel
           are bounded by the launch rate, not by HBM: the figure is an upper bound on the kernel's time.
  eval     one evaluation of SDEditEngine (strength 1: 50 evaluations) against the plain DenoiseEngine's 50 steps at the same batch,
           alternated pairs, ms per evaluation.
  call     one MyLDMPipeline.img2img_latents call, strength 0.6 of 50 steps (30 evaluations), batch 1 and 16, warm.

One JSON line per measurement.  `python tools/bench_img2img.py [--what kernel,eval,call] [--reps 4] [--dtype bf16]`;
`--kernel-only` launches each update a few times and exits (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sde import ffhq_unet  # noqa: E402

INF = float("inf")
# eta = 0 rows: "sdedit" mid row; "repaint" mid rows without and with the jump back up (the jump reads z_b too)
SDEDIT_ROW = (1.2, -0.5, -INF, INF, 0.9, 0.4, 0.0, 0.9, 0.43, 0.5, 0.0, 0.0)
REPAINT_ROWS = {"repaint": (1.2, -0.5, -INF, INF, 0.9, 0.4, 0.0, 0.9, 0.43, 1.0, 0.0, 0.0),
                "repaint_jump": (1.2, -0.5, -INF, INF, 0.9, 0.4, 0.0, 0.9, 0.43, 0.95, 0.31, 0.0)}


def bytes_per_element(kind, C, eps_bytes):
    """What one launch moves per latent element at eta = 0: fp32 x, the original / known latents, one noise (two on a jump row) and
    x_out, eps in the model's dtype, and the [B, 1, H, W] map or mask once per C elements."""
    fp32 = {"sdedit": 4, "repaint": 4, "repaint_jump": 5}[kind]
    return 4.0 * fp32 + eps_bytes + 4.0 / C


def kernel_calls(batch, dtype):
    from afldm_amd import ops
    C, S = 4, 32
    g = torch.Generator().manual_seed(0)
    x, orig, z = [torch.randn(batch, C, S, S, generator=g).cuda() for _ in range(3)]
    eps = torch.randn(batch, S, S, C, generator=g).to("cuda", dtype)
    m = (torch.randint(0, 5, (batch, 1, S, S), generator=g).float() / 4).cuda()
    noise3 = torch.randn(1, 3, batch, C, S, S, generator=g).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty_like(x)
    coefs = {k: torch.tensor(r, dtype=torch.float32).cuda() for k, r in dict(REPAINT_ROWS, sdedit=SDEDIT_ROW).items()}
    calls = {"sdedit": lambda: ops.sdedit_step(x, eps, orig, m, z, None, coefs["sdedit"], idx, out=out)}
    for k in REPAINT_ROWS:
        calls[k] = lambda k=k: ops.repaint_step(x, eps, orig, m, noise3, coefs[k], idx, out=out)
    return calls, x.numel()


def bench_kernel(a, dtype):
    for batch in (1, 8, 64):
        calls, n = kernel_calls(batch, dtype)
        times = {k: [] for k in calls}
        for fn in calls.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.launches):
                    fn()
                t1.record()
                t1.synchronize()
                times[k].append(t0.elapsed_time(t1) * 1e3 / a.launches)
        for k, ts in times.items():
            us = statistics.median(ts)
            nbytes = bytes_per_element(k, 4, 2 if dtype == torch.bfloat16 else 4) * n
            print(json.dumps({"what": "kernel", "kernel": k, "batch": batch, "dtype": a.dtype, "launches": a.launches,
                              "us_per_launch": round(us, 3), "runs_us": [round(t, 3) for t in ts], "bytes": int(nbytes),
                              "gbs": round(nbytes / us * 1e-3, 1), "hbm_frac": round(nbytes / us * 1e-6 / a.hbm_tbs, 4)}), flush=True)


def bench_eval(a, dtype, unet):
    from afldm_amd.engine import DenoiseEngine, SDEditEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    s = unet.config.sample_size
    for batch in (1, 8, 64):
        g = torch.Generator().manual_seed(0)
        x, orig, z = [torch.randn(batch, 4, s, s, generator=g) for _ in range(3)]
        cmap = torch.randint(0, 5, (1, 1, s, s), generator=g).float() / 4
        sch = ffhq_ddim_scheduler()
        plain = DenoiseEngine(unet, sch.schedule(50), batch, 50)
        sd = sch.sdedit_schedule(50, 1.0)
        edit = SDEditEngine(unet, sd, batch, 50)
        runs = {"plain": lambda: plain.run(x), "sdedit": lambda: edit.run(x, known=(orig, cmap, z))}
        times = {k: [] for k in runs}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / 50 * 1e3)
        p, e = statistics.median(times["plain"]), statistics.median(times["sdedit"])
        print(json.dumps({"what": "eval", "batch": batch, "dtype": a.dtype, "evaluations": 50, "plain_ms": round(p, 4),
                          "sdedit_ms": round(e, 4), "delta_us": round((e - p) * 1e3, 2), "delta_frac": round(e / p - 1, 5),
                          "pair_deltas_us": [round((u - v) * 1e3, 2) for u, v in zip(times["sdedit"], times["plain"])],
                          "plain_runs_ms": [round(t, 4) for t in times["plain"]],
                          "sdedit_runs_ms": [round(t, 4) for t in times["sdedit"]]}), flush=True)
        del plain, edit


def bench_call(a, dtype, unet):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    s = unet.config.sample_size
    for batch in (1, 16):
        g = torch.Generator().manual_seed(0)
        orig = 0.8 * torch.randn(batch, 4, s, s, generator=g)
        cmap = torch.linspace(0.0, 1.0, s).reshape(1, 1, 1, s).expand(1, 1, s, s).contiguous()

        def run():
            out = pipe.img2img_latents(orig, 0.6, cmap, 50, generator=torch.Generator().manual_seed(1))
            torch.cuda.synchronize()
            return out
        run()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        print(json.dumps({"what": "call", "batch": batch, "dtype": a.dtype, "strength": 0.6, "steps": 50, "evaluations": 30,
                          "call_ms": round(t * 1e3, 3), "ms_per_evaluation": round(t * 1e3 / 30, 4),
                          "runs_ms": [round(v * 1e3, 3) for v in ts]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--what", default="kernel,eval,call")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="peak HBM bandwidth in TB/s the fraction is taken of")
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    if not torch.cuda.is_available():
        raise SystemExit("bench_img2img needs an MI355X: there is no CPU path")
    if a.kernel_only:
        for batch in (1, 8, 64):
            calls, _ = kernel_calls(batch, dtype)
            for fn in calls.values():
                for _ in range(50):
                    fn()
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "batches": [1, 8, 64], "launches_each": 50}))
        return
    what = a.what.split(",")
    if "kernel" in what:
        bench_kernel(a, dtype)
    if "eval" in what or "call" in what:
        unet = ffhq_unet(dtype)
        if "eval" in what:
            bench_eval(a, dtype, unet)
        if "call" in what:
            bench_call(a, dtype, unet)


if __name__ == "__main__":
    main()
