#!/usr/bin/env python
"""FFHQ sampling with a step count per sample on MI355X - continuous batching (afldm_amd MyLDMPipeline.sample_mixed over
afldm_amd.serving.SamplingServer): every request has its own number of steps, the requests share the batch-`--slots`
replayed HIP graphs, and a slot that finishes takes the next request while its neighbours go on.

  --steps 20,35,50   the step counts; request i takes entry i mod 3 of the list
  --requests 12      how many samples
  --slots 4          batch rows of the replayed graph
  --solver dpm       DPM-Solver++ multistep instead of DDIM (about 20 steps do what 50 DDIM steps do); --solver-order 1 | 2 | 3

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture (demonstrates the full flow; the pictures
are noise).  Writes one PNG per sample."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ilvr_ffhq import build_pipeline  # noqa: E402  (the same pipeline sources: --ckpt or --random-init)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--output", type=str, default="results/mixed.png")
    p.add_argument("--steps", type=str, default="20,35,50", help="comma-separated step counts, cycled over the requests")
    p.add_argument("--requests", type=int, default=6)
    p.add_argument("--slots", type=int, default=4)
    p.add_argument("--engines", type=int, default=1, choices=[1, 2])
    p.add_argument("--solver", default="ddim", choices=["ddim", "dpm"], help="dpm: DPMSolverMultistepScheduler from the pipeline's config")
    p.add_argument("--solver-order", type=int, default=2, choices=[1, 2, 3], help="solver_order of --solver dpm")
    p.add_argument("--seed", type=int, default=1234)
    src = p.add_mutually_exclusive_group()
    src.add_argument("--ckpt", type=str, default=None)
    src.add_argument("--random-init", action="store_true", help="seeded random weights of the FFHQ architecture")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    args = p.parse_args(argv)
    if not args.random_init and not args.ckpt:
        args.ckpt = os.environ.get("AFLDM_CKPT")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt DIR or --random-init")
    args.steps = [int(s) for s in args.steps.split(",") if s.strip()]
    if not args.steps or min(args.steps) < 1 or args.requests < 1 or args.slots < 1:
        p.error("--steps, --requests and --slots must be >= 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    if args.solver == "dpm":
        from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
        pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, solver_order=args.solver_order)
    counts = [args.steps[i % len(args.steps)] for i in range(args.requests)]
    gens = [torch.Generator().manual_seed(args.seed + i) for i in range(args.requests)]
    out = pipe.sample_mixed(counts, generator=gens, output_type="pil", slots=args.slots, engines=args.engines)
    (server,) = pipe._slot_servers.values()
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    stem, ext = os.path.splitext(args.output)
    for i, im in enumerate(out.images):
        im.save(args.output if len(out.images) == 1 else f"{stem}_{i}{ext}")
    print(f"wrote {len(out.images)} image(s) to {args.output}: {args.solver} steps {counts} on {args.engines} x {args.slots} slots, "
          f"{server.replays} graph replays, {server.useful} of {server.evaluations} slot evaluations useful")
    return out.images


if __name__ == "__main__":
    main()
