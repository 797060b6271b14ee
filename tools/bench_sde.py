"""Wall time of the stochastic samplers on the graph-replayed engine against their eager loops (FFHQ-size UNet, random weights):

  * DDIM eta = 1, batch 64, 50 steps: MyLDMPipeline.__call__ with use_graph (afldm_sde_step) and with use_graph=False, with a
    CPU and with a CUDA generator; and the eta = 0 engine, for ms/step;
  * the I2SB bridge, stochastic and clipped, batch 32, 99 evaluations: I2SBLDMPipeline._bridge with and without use_graph.

Each configuration runs once to warm up (capture, packing, workspaces), then `--reps` timed runs, each ended by a device
synchronise; the median is printed.  One JSON line per configuration.
`python tools/bench_sde.py [--dtype bf16] [--reps 3] [--kernel-only]`; `--kernel-only` runs just a few steps of the eta = 0 and
eta = 1 engines (for a `rocprofv3 --kernel-trace --stats` run that compares afldm_sde_step with afldm_ddim_step)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ffhq_unet(dtype):
    from afldm_amd.af_modules.af_api import make_af_unet
    from afldm_amd.models.unet_2d import UNet2DModel
    from oracle import configs as oc, unet as ou
    unet = UNet2DModel.from_config(oc.FFHQ_UNET)
    unet.load_state_dict(ou.init_unet_params(oc.FFHQ_UNET, seed=0, conv_out_scale=0.1))
    make_af_unet(unet)
    return unet.to("cuda").to(dtype)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.schedulers.i2sb import I2SBScheduler
    unet = ffhq_unet(dtype)
    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    x = torch.randn(64, 4, 32, 32, generator=torch.Generator().manual_seed(0))

    if a.kernel_only:
        for eta in (0.0, 1.0):
            pipe(latents=x, eta=eta, num_inference_steps=10, generator=torch.Generator().manual_seed(1), output_type="latent")
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "batch": 64, "steps": 10}))
        return

    def ddim(eta, use_graph, gen):
        return lambda: pipe(latents=x, eta=eta, num_inference_steps=50, generator=gen() if gen else None,
                            output_type="latent", use_graph=use_graph)
    cpu = lambda: torch.Generator().manual_seed(1)                       # noqa: E731
    cuda = lambda: torch.Generator("cuda").manual_seed(1)                # noqa: E731
    det = timed(ddim(0.0, True, None), a.reps)
    rec = {"what": "ddim", "dtype": a.dtype, "batch": 64, "steps": 50, "eta0_graph_s": round(det, 4),
           "eta0_ms_per_step": round(det / 50 * 1e3, 3)}
    for name, gen in (("cpu_gen", cpu), ("cuda_gen", cuda)):
        g = timed(ddim(1.0, True, gen), a.reps)
        e = timed(ddim(1.0, False, gen), a.reps)
        rec[f"eta1_{name}_graph_s"] = round(g, 4)
        rec[f"eta1_{name}_eager_s"] = round(e, 4)
        rec[f"eta1_{name}_graph_ms_per_step"] = round(g / 50 * 1e3, 3)
        rec[f"eta1_{name}_speedup"] = round(e / g, 2)
    print(json.dumps(rec), flush=True)

    cfg = {k: v for k, v in FFHQ_DDIM_CONFIG.items() if k != "set_alpha_to_one"}
    sr = I2SBLDMPipeline(None, unet, I2SBScheduler.from_config(dict(cfg, clip_sample=True)))
    sr.set_progress_bar_config(disable=True)
    start = (0.8 * torch.randn(32, 4, 32, 32, generator=torch.Generator().manual_seed(2))).cuda()
    ode = I2SBLDMPipeline(None, unet, I2SBScheduler.from_config(cfg))
    ode.set_progress_bar_config(disable=True)
    rec = {"what": "i2sb", "dtype": a.dtype, "batch": 32, "evaluations": 99}
    rec["ode_unclipped_graph_s"] = round(timed(lambda: ode._bridge(start, 100, True, None), a.reps), 4)
    for name, gen in (("cpu_gen", cpu), ("cuda_gen", cuda)):
        g = timed(lambda: sr._bridge(start, 100, False, gen()), a.reps)
        e = timed(lambda: sr._bridge(start, 100, False, gen(), use_graph=False), a.reps)
        rec[f"sde_clipped_{name}_graph_s"] = round(g, 4)
        rec[f"sde_clipped_{name}_eager_s"] = round(e, 4)
        rec[f"sde_clipped_{name}_speedup"] = round(e / g, 2)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
