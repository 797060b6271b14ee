#!/usr/bin/env python
"""FFHQ sampling in parallel over the time axis on MI355X - ParaDiGMS (Shih et al., NeurIPS 2023) on the unconditional FFHQ
latent-diffusion model (afldm_amd MyLDMPipeline.sample_parallel): --window consecutive DDIM steps of an image are evaluated as ONE
UNet batch and iterated to their fixed point, every iteration ending in afldm_picard_sweep / _stride / _slide on replayed HIP
graphs.  A sample costs `iterations` evaluations of batch --window instead of --steps evaluations of batch 1; --tolerance 0 is
the plain DDIM sampler (one state accepted per iteration), a larger tolerance accepts more states per iteration and moves the
sample away from the sequential one.

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture (demonstrates the full flow; the picture
is noise, and the iteration count says nothing about a trained model).  Writes one PNG per sample.

--timings: no picture.  In one process, after a warm-up of each, the parallel sampler at --tolerance, the parallel sampler at
tolerance 0 and the plain sampler (MyLDMPipeline.__call__) at batch --batch ALTERNATE `--reps` times, each run ended by a device
synchronise.  Prints one JSON line with the medians, every run, the iteration counts and a fingerprint of the box.
tools/bench_picard.py measures the iteration itself."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", "--output", dest="out", type=str, default="results/parallel.png")
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--window", type=int, default=8, help="steps evaluated as one UNet batch per image")
    p.add_argument("--tolerance", type=float, default=0.1, help="root-mean-square change below which a state is accepted; 0: DDIM exactly")
    p.add_argument("--seed", type=int, default=1234)
    src = p.add_mutually_exclusive_group()
    src.add_argument("--ckpt", type=str, default=None)
    src.add_argument("--random-init", action="store_true", help="seeded random weights of the FFHQ architecture")
    p.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the torch loop instead of replayed HIP graphs")
    p.add_argument("--timings", action="store_true", help="measure instead of writing a picture (see the module docstring)")
    p.add_argument("--reps", type=int, default=5)
    args = p.parse_args(argv)
    if not args.random_init and not args.ckpt:
        args.ckpt = os.environ.get("AFLDM_CKPT")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt DIR or --random-init")
    if args.steps < 1 or args.reps < 1 or args.batch < 1 or args.window < 1 or args.tolerance < 0:
        p.error("--steps, --reps, --batch and --window must be >= 1 and --tolerance >= 0")
    return args


def timings(args, pipe):
    from panorama_ffhq import box_fingerprint
    c, s = pipe.unet.config.in_channels, pipe.unet.config.sample_size
    x = torch.randn(args.batch, c, s, s, generator=torch.Generator().manual_seed(args.seed))
    counts = {}

    def parallel(name, tolerance):
        own = type(pipe)(None, pipe.unet, pipe.scheduler)                # a pipeline keeps ONE engine per sampler: one per tolerance
        own.set_progress_bar_config(disable=True)

        def run():
            _, stats = own.sample_parallel_latents(latents=x, num_inference_steps=args.steps, window=args.window, tolerance=tolerance)
            counts[name] = stats["iterations"]
        return run

    runs = {"parallel": parallel("parallel", args.tolerance),
            "parallel_tolerance_0": parallel("parallel_tolerance_0", 0.0),
            "sampler": lambda: pipe(latents=x, num_inference_steps=args.steps, output_type="latent")}
    wall = {k: [] for k in runs}
    for fn in runs.values():                                               # warm-up: capture, packing, workspaces
        fn()
        torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
    out = {"what": "sample_parallel", "dtype": args.dtype, "batch": args.batch, "steps": args.steps, "window": args.window,
           "tolerance": args.tolerance, "reps": args.reps, "iterations": counts, "random_weights": bool(args.random_init)}
    for k, ts in wall.items():
        out[k + "_s"] = round(statistics.median(ts), 4)
        out[k + "_runs_s"] = [round(t, 4) for t in ts]
    out["box"] = box_fingerprint()
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    from panorama_ffhq import build_pipeline
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args, with_vae=not args.timings).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    if pipe.vae is not None:
        make_af_vae_from_config(pipe.vae)
    if args.timings:
        return timings(args, pipe)
    out = pipe.sample_parallel(args.batch, args.steps, args.window, args.tolerance, generator=torch.Generator().manual_seed(args.seed),
                               use_graph=not args.eager, output_type="pil")
    stats = pipe.parallel_stats
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    stem, ext = os.path.splitext(args.out)
    for i, im in enumerate(out.images):
        im.save(args.out if len(out.images) == 1 else f"{stem}_{i}{ext}")
    print(f"wrote {len(out.images)} image(s) to {args.out}: {args.steps} steps in {stats['iterations']} iterations of a window of "
          f"{args.window} at tolerance {args.tolerance} ({stats['evaluations']} UNet rows evaluated)")
    return out.images


if __name__ == "__main__":
    main()
