#!/usr/bin/env python
"""FFHQ inpainting on MI355X — RePaint (Lugmayr et al., CVPR 2022; the options of diffusers' RePaintPipeline: steps, eta,
jump_length, jump_n_sample) on the unconditional FFHQ latent-diffusion model (afldm_amd MyLDMPipeline.inpaint: VAE-encode the
image, pool the mask to the latent grid, resample the masked-out part on replayed HIP graphs, decode, composite).

The mask is a PNG (or any image PIL reads) of the image's size: white = keep, black = generate; --invert-mask swaps them.

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture, a seeded synthetic image and a centred
square hole (demonstrates the full flow; the pictures are noise).  Writes one PNG."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--input_path", type=str, default=None)
    p.add_argument("--mask_path", type=str, default=None, help="white = keep, black = generate")
    p.add_argument("--invert-mask", action="store_true", help="white = generate, black = keep")
    p.add_argument("--output_path", type=str, default="results/inpaint.png")
    p.add_argument("--n_steps", type=int, default=50)
    p.add_argument("--jump_length", type=int, default=10)
    p.add_argument("--jump_n_sample", type=int, default=10)
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--mask-mode", default="min", choices=["min", "mean"],
                   help="how the pixel mask reaches the latent grid: a latent is kept only if every pixel under it is (min), or "
                        "the kept fraction as a soft mask (mean)")
    p.add_argument("--no-composite", action="store_true", help="write the decoded sample itself instead of pasting the kept pixels")
    p.add_argument("--ckpt", type=str, default=os.environ.get("AFLDM_CKPT"))
    p.add_argument("--random-init", action="store_true",
                   help="seeded random weights of the FFHQ architecture, a synthetic image and a centred square hole")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the eager loop instead of replayed HIP graphs")
    args = p.parse_args(argv)
    if not args.random_init and not (args.input_path and args.mask_path):
        p.error("pass --input_path and --mask_path (or --random-init for a synthetic image and mask)")
    if args.jump_length < 1 or args.jump_n_sample < 1 or args.n_steps < 1:
        p.error("--n_steps, --jump_length and --jump_n_sample must be >= 1")
    return args


def synthetic_inputs(seed, size):
    """A smooth seeded [1, 3, size, size] image in [-1, 1] and a mask [1, 1, size, size] with a centred square hole."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, 3, 8, 8, generator=g) * 2 - 1
    image = torch.nn.functional.interpolate(x, size=(size, size), mode="bicubic", align_corners=False).clamp(-1, 1)
    mask = torch.ones(1, 1, size, size)
    mask[..., size // 4: 3 * size // 4, size // 4: 3 * size // 4] = 0.0
    return image, mask


def load_mask(path, size, invert=False):
    """[1, 1, size, size] in {0, 1}: 1 where the (nearest-resized, grey) mask image is brighter than mid-grey."""
    import numpy as np
    from PIL import Image
    img = Image.open(path).convert("L").resize((size, size), Image.NEAREST)
    m = torch.from_numpy((np.asarray(img, dtype=np.float32) / 255.0 > 0.5).astype(np.float32))[None, None]
    return 1.0 - m if invert else m


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
    if args.random_init:
        image, mask = synthetic_inputs(args.seed, size)
    else:
        image = image_to_tensor(args.input_path, resolution=(size, size))
        mask = load_mask(args.mask_path, size, args.invert_mask)
    out = pipe.inpaint(image, mask, num_inference_steps=args.n_steps, eta=args.eta, jump_length=args.jump_length,
                       jump_n_sample=args.jump_n_sample, generator=torch.Generator().manual_seed(args.seed),
                       use_graph=not args.eager, mask_mode=args.mask_mode, composite=not args.no_composite, output_type="pil")
    d = os.path.dirname(args.output_path)
    if d:
        os.makedirs(d, exist_ok=True)
    out.images[0].save(args.output_path)
    kept = float(mask.mean())
    print(f"wrote {args.output_path}: {size} x {size}, {100 * (1 - kept):.1f} % of the pixels generated")
    return out.images[0]


if __name__ == "__main__":
    main()
