#!/usr/bin/env python
"""FFHQ two-image interpolation on MI355X — the options of the reference's scripts/image_interpolation.py (--input_path_1
--input_path_2 --output_path --n_frames --n_steps) on the unconditional FFHQ model (afldm_amd LDMInterpolationPipeline:
DDIM inversion of both images, slerp of the inverted latents, two STORE passes, one LOAD pass blending both).

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture and two seeded synthetic images
(demonstrates the full flow; the pictures are noise).  Writes the frames as one GIF."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--input_path_1", type=str, default=None)
    p.add_argument("--input_path_2", type=str, default=None)
    p.add_argument("--output_path", type=str, default="results/interp.gif")
    p.add_argument("--n_frames", type=int, default=17)
    p.add_argument("--n_steps", type=int, default=50)
    p.add_argument("--ckpt", type=str, default=os.environ.get("AFLDM_CKPT"))
    p.add_argument("--random-init", action="store_true",
                   help="seeded random weights of the FFHQ architecture and two seeded synthetic images (no checkpoint needed)")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--seed", type=int, default=1234,
                   help="seeds the synthetic images of --random-init and the random draws of --warp-method 0-2")
    p.add_argument("--eager", action="store_true",
                   help="run the passes as the eager loop that follows the reference statement by statement instead of replayed "
                        "HIP graphs")
    p.add_argument("--warp-method", type=int, default=3, choices=[0, 1, 2, 3],
                   help="how intermediate frames start (reference image_interpolation_pipeline.py:556-599): 0 = up-sampled noise "
                        "forward-warped along the flow (the reference script's choice), 1 = conditional noise up-sampling + warp, "
                        "2 = the latents warped, 3 = slerp only; 0-2 need --flow")
    p.add_argument("--flow", type=str, default=None, metavar="FILE.npz | estimate",
                   help="optical flow between the two images from any estimator: arrays `fwd` and `bwd`, each [2, S, S] or "
                        "[1, 2, S, S] at the image size, channel 0 = x displacement (GMFlow's output convention); or the word "
                        "`estimate`: the built-in pyramidal Lucas-Kanade estimator (shift_utils.flow_estimation.PyramidLKFlow: "
                        "a classical estimator, not GMFlow)")
    args = p.parse_args(argv)
    if args.warp_method != 3 and not args.flow:
        p.error("--warp-method 0, 1 and 2 warp along optical flow: pass --flow FILE.npz (arrays fwd, bwd) or --flow estimate")
    if args.n_frames < 2:
        p.error("--n_frames must be >= 2")
    if not args.random_init and not (args.input_path_1 and args.input_path_2):
        p.error("pass --input_path_1 and --input_path_2 (or --random-init for synthetic images)")
    return args


def synthetic_images(seed, size=256):
    """Two smooth seeded [1, 3, size, size] images in [-1, 1] (random 8 x 8 colour fields, bicubic-upsampled)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        x = torch.rand(1, 3, 8, 8, generator=g) * 2 - 1
        out.append(torch.nn.functional.interpolate(x, size=(size, size), mode="bicubic", align_corners=False).clamp(-1, 1))
    return out


def load_flows(path):
    """(fwd_flow, bwd_flow) fp32 [1, 2, S, S] from the arrays `fwd` and `bwd` of an .npz file."""
    import numpy as np
    with np.load(path) as z:
        missing = [k for k in ("fwd", "bwd") if k not in z.files]
        if missing:
            raise SystemExit(f"{path}: array(s) {missing} missing (found {z.files})")
        out = []
        for k in ("fwd", "bwd"):
            f = torch.from_numpy(np.asarray(z[k], dtype=np.float32))
            out.append(f[None] if f.dim() == 3 else f)
    return tuple(out)


def flow_source(pipe, flow):
    """What --flow asks for: `estimate` hands the pipeline the built-in estimator (it then estimates the flows itself: None is
    returned), a file gives the caller's (fwd_flow, bwd_flow), nothing gives None."""
    if flow == "estimate":
        from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow
        pipe.flow_model = PyramidLKFlow()
        return None
    return load_flows(flow) if flow else None


def build_pipeline(args):
    from afldm_amd.pipelines.image_interpolation_pipeline import LDMInterpolationPipeline
    if args.ckpt:
        return LDMInterpolationPipeline.from_pretrained(args.ckpt)
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
    return LDMInterpolationPipeline(vae, unet, DDIMScheduler.from_config(FFHQ_DDIM_CONFIG))


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    from afldm_amd.io_utils import save_gif_from_tensors
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    if args.random_init:
        image1, image2 = synthetic_images(args.seed)
    else:
        image1, image2 = args.input_path_1, args.input_path_2
    flows = flow_source(pipe, args.flow)
    frames = pipe(image1, image2, num_frames=args.n_frames, num_inference_steps=args.n_steps, output_type="pt",
                  use_graph=not args.eager, warp_method=args.warp_method, flows=flows,
                  generator=torch.Generator().manual_seed(args.seed))
    save_gif_from_tensors(list(frames.float().cpu()), args.output_path, denorm=True)
    print(f"wrote {args.output_path}: {frames.shape[0]} frames of {tuple(frames.shape[1:])}")
    return frames


if __name__ == "__main__":
    main()
