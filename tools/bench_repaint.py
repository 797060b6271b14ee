"""Wall time of RePaint inpainting on the graph-replayed engine against its eager loop (FFHQ-size UNet, random weights):
MyLDMPipeline.inpaint_latents with (num_inference_steps, jump_length, jump_n_sample) = (50, 10, 10) - 410 UNet evaluations - at
batch 1 and batch 16, half of the latent kept, with a CPU generator.

Each configuration runs once to warm up (capture, packing, workspaces); then graph and eager runs ALTERNATE `--reps` times, each ended
by a device synchronise, and the medians are printed: one JSON line per batch size.
`python tools/bench_repaint.py [--dtype bf16] [--reps 3] [--batches 1,16] [--kernel-only]`; `--kernel-only` runs a few evaluations of
the DDIM engine and of the RePaint engine at batch 64 as eager dispatches (for a `rocprofv3 --kernel-trace --stats` run that compares
k_repaint_step with k_ddim_step)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_sde import ffhq_unet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--steps", default="50,10,10", help="num_inference_steps,jump_length,jump_n_sample")
    ap.add_argument("--eta", type=float, default=0.0)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = ffhq_unet(dtype)
    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    s = unet.config.sample_size

    def inputs(batch):
        g = torch.Generator().manual_seed(0)
        x = torch.randn(batch, 4, s, s, generator=g)
        known = 0.8 * torch.randn(batch, 4, s, s, generator=g)
        mask = torch.zeros(1, 1, s, s)
        mask[..., : s // 2] = 1.0
        return x, known, mask

    if a.kernel_only:
        x, known, mask = inputs(64)
        sched = ffhq_ddim_scheduler()
        DenoiseEngine(unet, sched.schedule(10), 64, 10, use_graph=False).run(x)
        rp = sched.repaint_schedule(6, 0.7, 2, 2)                         # 10 evaluations, every slot in use somewhere
        eng = DenoiseEngine(unet, rp, 64, len(rp.timesteps), use_graph=False)
        eng.run(x, draw=rp.drawer(torch.Generator("cuda").manual_seed(1), tuple(x.shape), unet.device, unet.dtype),
                known=(known.cuda(), mask.cuda()))
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "batch": 64, "ddim_steps": 10, "repaint_evaluations": len(rp.timesteps)}))
        return

    n, jl, js = (int(v) for v in a.steps.split(","))
    for batch in (int(b) for b in a.batches.split(",")):
        x, known, mask = inputs(batch)

        def run(use_graph):
            out = pipe.inpaint_latents(known, mask, num_inference_steps=n, eta=a.eta, jump_length=jl, jump_n_sample=js, latents=x,
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
        evals = len(pipe.scheduler.repaint_schedule(n, a.eta, jl, js).timesteps)
        g, e = statistics.median(tg), statistics.median(te)
        print(json.dumps({"what": "repaint", "dtype": a.dtype, "batch": batch, "steps": [n, jl, js], "eta": a.eta,
                          "evaluations": evals, "graph_s": round(g, 4), "eager_s": round(e, 4),
                          "graph_ms_per_evaluation": round(g / evals * 1e3, 3), "eager_ms_per_evaluation": round(e / evals * 1e3, 3),
                          "speedup": round(e / g, 2), "graph_runs_s": [round(t, 4) for t in tg],
                          "eager_runs_s": [round(t, 4) for t in te]}), flush=True)


if __name__ == "__main__":
    main()
