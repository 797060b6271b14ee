#!/usr/bin/env python
"""FFHQ sampling with self-attention guidance on MI355X - SAG (Hong et al., ICCV 2023; diffusers StableDiffusionSAGPipeline) on the
unconditional FFHQ latent-diffusion model (afldm_amd MyLDMPipeline.sag: every step evaluates the UNet, reads how much attention
each token of ONE self-attention site receives, blurs the predicted image where that mass exceeds 1, re-noises it, evaluates the
UNet again on the result and steers away from that second prediction, all on replayed HIP graphs; decode).
--sag-scale is the guidance scale s, --guidance-rescale pulls the guided prediction's standard deviation back towards the plain
one's (diffusers' rescale_noise_cfg), --site names the attention block: a module path, or a prefix of one on a '.' boundary that
selects exactly one.  It defaults to up_blocks.2.attentions.0, the 8 x 8 up-block attention (64 tokens, each covering 4 x 4
latents): diffusers' "mid_block" is the 2 x 2 level on this model, a map of 4 tokens.

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
    p.add_argument("--output", type=str, default="results/sag.png")
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--sag-scale", type=float, default=0.75)
    p.add_argument("--site", type=str, default="up_blocks.2.attentions.0", help="the attention block whose map is read")
    p.add_argument("--blur-kernel-size", type=int, default=9)
    p.add_argument("--blur-sigma", type=float, default=1.0)
    p.add_argument("--blur-boundary", default="reflect", choices=["reflect", "circular"])
    p.add_argument("--guidance-rescale", type=float, default=0.0)
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--seed", type=int, default=1234)
    src = p.add_mutually_exclusive_group()
    src.add_argument("--ckpt", type=str, default=None)
    src.add_argument("--random-init", action="store_true", help="seeded random weights of the FFHQ architecture")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the eager loop instead of replayed HIP graphs")
    args = p.parse_args(argv)
    if not args.random_init and not args.ckpt:
        args.ckpt = os.environ.get("AFLDM_CKPT")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt DIR or --random-init")
    if args.sag_scale < 0 or not 0 <= args.guidance_rescale <= 1 or args.steps < 1 or args.batch_size < 1:
        p.error("--sag-scale must be >= 0, --guidance-rescale in [0, 1], --steps and --batch-size >= 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    out = pipe.sag(batch_size=args.batch_size, sag_scale=args.sag_scale, sag_site=args.site, blur_kernel_size=args.blur_kernel_size,
                   blur_sigma=args.blur_sigma, blur_boundary=args.blur_boundary, guidance_rescale=args.guidance_rescale,
                   eta=args.eta, num_inference_steps=args.steps, generator=torch.Generator().manual_seed(args.seed),
                   use_graph=not args.eager, output_type="pil")
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    stem, ext = os.path.splitext(args.output)
    for i, im in enumerate(out.images):
        im.save(args.output if len(out.images) == 1 else f"{stem}_{i}{ext}")
    print(f"wrote {len(out.images)} image(s) to {args.output}: sag_scale {args.sag_scale}, site {pipe.sag_site_of(args.site)}, "
          f"{args.blur_kernel_size} taps, sigma {args.blur_sigma}, {args.blur_boundary} boundary, guidance_rescale {args.guidance_rescale}")
    return out.images


if __name__ == "__main__":
    main()
