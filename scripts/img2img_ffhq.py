#!/usr/bin/env python
"""FFHQ image-to-image on MI355X — SDEdit (Meng et al., ICLR 2022) with a per-pixel change map (Differential Diffusion, Levin &
Fried 2023) on the unconditional FFHQ latent-diffusion model (afldm_amd MyLDMPipeline.img2img: VAE-encode the image, pool the
change map to the latent grid, noise the latents to the chosen strength, denoise on replayed HIP graphs while every element is
held on the original's noised trajectory until the schedule reaches its change value, decode, composite).

The change map is a grey image (or any image PIL reads) of the image's size: black = keep exactly, white = regenerate at the full
--strength, grey levels between.  --ramp makes a left-to-right ramp instead (the left edge kept, the right edge regenerated);
without either the whole image changes by --strength (plain SDEdit).

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture and a seeded synthetic image
(demonstrates the full flow; the pictures are noise).  Writes one PNG."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--image", type=str, default=None)
    p.add_argument("--strength", type=float, default=0.6, help="how far the image is noised: the last int(n_steps * strength) steps run")
    m = p.add_mutually_exclusive_group()
    m.add_argument("--change-map", type=str, default=None, metavar="FILE", help="black = keep, white = regenerate")
    m.add_argument("--ramp", action="store_true", help="a left-to-right ramp as the change map")
    p.add_argument("--output_path", type=str, default="results/img2img.png")
    p.add_argument("--n_steps", type=int, default=50)
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--no-composite", action="store_true", help="write the decoded sample itself instead of pasting the kept pixels")
    p.add_argument("--ckpt", type=str, default=os.environ.get("AFLDM_CKPT"))
    p.add_argument("--random-init", action="store_true", help="seeded random weights of the FFHQ architecture and a synthetic image")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the eager loop instead of replayed HIP graphs")
    args = p.parse_args(argv)
    if not args.random_init and not args.image:
        p.error("pass --image (or --random-init for a synthetic image)")
    if not 0.0 <= args.strength <= 1.0:
        p.error("--strength must be in [0, 1]")
    if args.n_steps < 1 or int(args.n_steps * args.strength) < 1:
        p.error("--n_steps must be >= 1 and int(n_steps * strength) >= 1: nothing would run")
    return args


def synthetic_image(seed, size):
    """A smooth seeded [1, 3, size, size] image in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, 3, 8, 8, generator=g) * 2 - 1
    return torch.nn.functional.interpolate(x, size=(size, size), mode="bicubic", align_corners=False).clamp(-1, 1)


def ramp_map(size):
    """[1, 1, size, size]: 0 in the left-most column, 1 in the right-most, linear between."""
    return torch.linspace(0.0, 1.0, size).reshape(1, 1, 1, size).expand(1, 1, size, size).contiguous()


def load_change_map(path, size):
    """[1, 1, size, size] in [0, 1]: the (bilinearly resized, grey) image's brightness."""
    import numpy as np
    from PIL import Image
    img = Image.open(path).convert("L").resize((size, size), Image.BILINEAR)
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0)[None, None].contiguous()


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
    image = synthetic_image(args.seed, size) if args.random_init and not args.image else image_to_tensor(args.image, resolution=(size, size))
    cmap = ramp_map(size) if args.ramp else (load_change_map(args.change_map, size) if args.change_map else None)
    out = pipe.img2img(image, strength=args.strength, change_map=cmap, num_inference_steps=args.n_steps, eta=args.eta,
                       generator=torch.Generator().manual_seed(args.seed), use_graph=not args.eager,
                       composite=not args.no_composite, output_type="pil")
    d = os.path.dirname(args.output_path)
    if d:
        os.makedirs(d, exist_ok=True)
    out.images[0].save(args.output_path)
    kept = 0.0 if cmap is None else float((cmap == 0).float().mean())
    print(f"wrote {args.output_path}: {size} x {size}, strength {args.strength} ({int(args.n_steps * args.strength)} of {args.n_steps} "
          f"steps), {100 * kept:.1f} % of the pixels kept exactly")
    return out.images[0]


if __name__ == "__main__":
    main()
