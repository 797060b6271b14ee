#!/usr/bin/env python
"""Reference-guided FFHQ sampling on MI355X - ILVR (Choi et al., ICCV 2021, Algorithm 1) on the unconditional FFHQ
latent-diffusion model (afldm_amd MyLDMPipeline.ilvr: VAE-encode the reference image, sample latents whose low band is the
reference's on replayed HIP graphs, decode).  --down-factor N sets the band that is kept: the ideal low-pass of cut-off 1 / N on
the 32 x 32 latent grid (2, 4, 8 keep 15, 7, 3 frequencies per axis); --range-t stops the guidance below that timestep.

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture and, without --image, a seeded synthetic
reference (demonstrates the full flow; the pictures are noise).  Writes one PNG."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--image", type=str, default=None, help="the reference image")
    p.add_argument("--output", type=str, default="results/ilvr.png")
    p.add_argument("--down-factor", type=float, default=4, help="N of phi_N: the low-pass cut-off is 1 / N")
    p.add_argument("--range-t", type=int, default=0, help="guide while the timestep is above this")
    p.add_argument("--eta", type=float, default=1.0)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--seed", type=int, default=1234)
    src = p.add_mutually_exclusive_group()
    src.add_argument("--ckpt", type=str, default=None)
    src.add_argument("--random-init", action="store_true",
                     help="seeded random weights of the FFHQ architecture (and a synthetic reference without --image)")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the eager loop instead of replayed HIP graphs")
    args = p.parse_args(argv)
    if not args.random_init and not args.ckpt:
        args.ckpt = os.environ.get("AFLDM_CKPT")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt DIR or --random-init")
    if not args.random_init and not args.image:
        p.error("pass --image (or --random-init for a synthetic reference)")
    if args.down_factor <= 0 or args.steps < 1:
        p.error("--down-factor must be > 0 and --steps >= 1")
    if args.down_factor == int(args.down_factor):
        args.down_factor = int(args.down_factor)
    return args


def synthetic_image(seed, size):
    """A smooth seeded [1, 3, size, size] image in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, 3, 8, 8, generator=g) * 2 - 1
    return torch.nn.functional.interpolate(x, size=(size, size), mode="bicubic", align_corners=False).clamp(-1, 1)


def build_pipeline(args):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    if args.ckpt:
        return MyLDMPipeline.from_pretrained(args.ckpt)
    from afldm_amd.configs import FFHQ_DDIM_CONFIG, FFHQ_UNET_CONFIG
    from afldm_amd.models.unet_2d import UNet2DModel
    from afldm_amd.models.vae import AutoencoderKL
    from afldm_amd.schedulers.ddim import DDIMScheduler
    torch.manual_seed(0)
    unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG)
    with torch.no_grad():
        unet.conv_out.weight.mul_(0.1)
        unet.conv_out.bias.mul_(0.1)
    vae = AutoencoderKL(in_channels=3, out_channels=3, down_block_types=["DownEncoderBlock2D"] * 4,
                        up_block_types=["UpDecoderBlock2D"] * 4, block_out_channels=[128, 256, 512, 512],
                        layers_per_block=2, latent_channels=4, scaling_factor=0.6, mid_act=True,
                        down_filtered_act=[False, True, True, True], up_filtered_act=[True, True, True, False],
                        up_rescale=[True, True, True])
    return MyLDMPipeline(vae, unet, DDIMScheduler.from_config(FFHQ_DDIM_CONFIG))


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    from afldm_amd.io_utils import image_to_tensor
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    size = pipe.unet.config.sample_size * 2 ** (len(pipe.vae.config.block_out_channels) - 1)
    image = image_to_tensor(args.image, resolution=(size, size)) if args.image else synthetic_image(args.seed, size)
    out = pipe.ilvr(image, down_factor=args.down_factor, range_t=args.range_t, num_inference_steps=args.steps, eta=args.eta,
                    generator=torch.Generator().manual_seed(args.seed), use_graph=not args.eager, output_type="pil")
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    out.images[0].save(args.output)
    print(f"wrote {args.output}: {size} x {size}, down factor {args.down_factor}, guided above timestep {args.range_t}")
    return out.images[0]


if __name__ == "__main__":
    main()
