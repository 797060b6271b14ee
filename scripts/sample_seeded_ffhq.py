#!/usr/bin/env python
"""FFHQ sampling with seeded stochastic DDIM on MI355X (afldm_amd MyLDMPipeline.sample_seeded): one sample per seed, the noise
of every step a function of (seed, step, element) that the update kernel computes in registers - Philox-4x32-10 and Box-Muller,
include/afldm_hip_noise.h - so there is no noise buffer and no host draw, and a seed gives the same picture in any batch.

  --seeds 1,2,3,4    one sample per seed (integers in [0, 2^63))
  --eta 1.0          DDIM's eta; 0 is the deterministic sampler from the same start latents
  --steps 50
  --mixed 20,35,50   instead: one request per seed through the slot sampler (sample_mixed), request i with entry i mod 3 of these
                     step counts - stochastic requests of different lengths sharing one replayed batch of --slots rows

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
    p.add_argument("--output", type=str, default="results/seeded.png")
    p.add_argument("--seeds", type=str, default="1,2,3,4")
    p.add_argument("--eta", type=float, default=1.0)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--mixed", type=str, default=None, help="comma-separated step counts, cycled over the seeds: serve them in slots")
    p.add_argument("--slots", type=int, default=4)
    p.add_argument("--eager", action="store_true", help="the eager loop (afldm_counter_noise + afldm_sde_step) instead of replayed graphs")
    src = p.add_mutually_exclusive_group()
    src.add_argument("--ckpt", type=str, default=None)
    src.add_argument("--random-init", action="store_true", help="seeded random weights of the FFHQ architecture")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    args = p.parse_args(argv)
    if not args.random_init and not args.ckpt:
        args.ckpt = os.environ.get("AFLDM_CKPT")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt DIR or --random-init")
    args.seeds = [int(s) for s in args.seeds.split(",") if s.strip()]
    args.mixed = [int(s) for s in args.mixed.split(",") if s.strip()] if args.mixed else None
    if not args.seeds or min(args.seeds) < 0 or max(args.seeds) >= 2 ** 63 or args.steps < 1 or args.slots < 1:
        p.error("--seeds: integers in [0, 2^63); --steps and --slots must be >= 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    if args.mixed:
        counts = [args.mixed[i % len(args.mixed)] for i in range(len(args.seeds))]
        out = pipe.sample_mixed(counts, output_type="pil", slots=args.slots, eta=args.eta, seeds=args.seeds)
        what = f"steps {counts} on {args.slots} slots"
    else:
        out = pipe.sample_seeded(args.seeds, eta=args.eta, num_inference_steps=args.steps, use_graph=not args.eager, output_type="pil")
        what = f"{args.steps} steps"
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    stem, ext = os.path.splitext(args.output)
    for seed, im in zip(args.seeds, out.images):
        im.save(args.output if len(out.images) == 1 else f"{stem}_{seed}{ext}")
    print(f"wrote {len(out.images)} image(s) to {args.output}: seeds {args.seeds}, eta {args.eta}, {what}")
    return out.images


if __name__ == "__main__":
    main()
