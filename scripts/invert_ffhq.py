#!/usr/bin/env python
"""FFHQ exact inversion on MI355X — the bit-reversible sampler (afldm_amd MyLDMPipeline.invert_reversible / sample_reversible: a
two-step form of DDIM after BDIA, Zhang et al., ECCV 2024, at gamma = 1, on int64 fixed-point latents).

With an image: VAE-encode it, invert the latents to a code at the noise end (or, with --strength, part of the way), sample back
from the code, and compare.  With --from-noise: sample from seeded noise, invert the result, and compare with the noise.  Prints
the number of latent integers that differ between the start and the round trip (expected: 0) and the PSNR of the decoded round
trip against the AF-VAE's own reconstruction of the start (with 0 differing integers the two decodes see the same latents).

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture and a seeded synthetic image."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    m = p.add_mutually_exclusive_group()
    m.add_argument("--image", type=str, default=None)
    m.add_argument("--from-noise", action="store_true", help="sample from seeded noise and invert back to it")
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--strength", type=float, default=None, help="invert up the first int(steps * strength) levels only")
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--ckpt", type=str, default=os.environ.get("AFLDM_CKPT"))
    p.add_argument("--random-init", action="store_true", help="seeded random weights of the FFHQ architecture and a synthetic image")
    p.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the eager loop instead of replayed HIP graphs")
    args = p.parse_args(argv)
    if not args.ckpt and not args.random_init:
        p.error("pass --ckpt DIR or --random-init")
    if not args.random_init and not args.image and not args.from_noise:
        p.error("pass an --image or --from-noise (or --random-init for a synthetic image)")
    if args.steps < 2:
        p.error("--steps must be >= 2: a code holds two levels")
    if args.strength is not None:
        if args.from_noise:
            p.error("--strength goes with an image: sampling from noise starts at the last level")
        if not 0.0 <= args.strength <= 1.0 or int(args.steps * args.strength) < 2:
            p.error("--strength must be in [0, 1] with int(steps * strength) >= 2")
    return args


def psnr(a, b):
    """PSNR in dB of two tensors in [-1, 1] (peak-to-peak 2); inf for equal tensors."""
    mse = float((a.double() - b.double()).pow(2).mean())
    return math.inf if mse == 0.0 else 10.0 * math.log10(4.0 / mse)


def main(argv=None):
    args = parse_args(argv)
    from img2img_ffhq import build_pipeline, synthetic_image
    from afldm_amd import ops
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    from afldm_amd.io_utils import image_to_tensor
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    c, s = pipe.unet.config.in_channels, pipe.unet.config.sample_size
    graph = not args.eager
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    if args.from_noise:
        noise = torch.randn(1, c, s, s, generator=torch.Generator().manual_seed(args.seed))
        start = ops.rev_encode(noise.to("cuda", dtype).float().contiguous(), bad)
        _, code = pipe.sample_reversible_latents(latents=noise.to(dtype), num_inference_steps=args.steps, use_graph=graph, return_code=True)
        back = pipe.invert_reversible(code=code, num_inference_steps=args.steps, use_graph=graph).hi
    else:
        size = s * 2 ** (len(pipe.vae.config.block_out_channels) - 1)
        image = synthetic_image(args.seed, size) if not args.image else image_to_tensor(args.image, resolution=(size, size))
        latents = pipe._encode_mode(image).float().contiguous()
        start = ops.rev_encode(latents, bad)
        code = pipe.invert_reversible(latents, num_inference_steps=args.steps, strength=args.strength, use_graph=graph)
        back = pipe.sample_reversible_latents(code=code, num_inference_steps=args.steps, use_graph=graph, return_code=True)[1].lo
    differing = int((back != start).sum())
    from afldm_amd.reversible import decode

    def pixels(X):
        return pipe.vae.decode(decode(X).to(pipe.vae.dtype) / pipe.vae.config.scaling_factor).sample.float()
    db = psnr(pixels(back), pixels(start))
    print(f"{args.steps} steps" + (f", strength {args.strength}" if args.strength is not None else "") +
          f", {args.dtype}, {'eager' if args.eager else 'graph'}: {differing} of {start.numel()} latent integers differ (expected 0); "
          f"PSNR of the decoded round trip against the AF-VAE reconstruction {db:.2f} dB")
    return differing, db


if __name__ == "__main__":
    main()
