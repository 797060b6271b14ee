#!/usr/bin/env python
"""FFHQ fractional-shift equivariance demo on MI355X — same CLI as the reference's
scripts/shift_ldm_ffhq.py (--num_inference_steps --shift_steps --output_path --input_path).

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format
directory with unet/, scheduler/, vae/) or --random-init for seeded random weights of the FFHQ
architecture (demonstrates the full flow; the picture is noise).  Multi-GPU: launch with
torch.distributed.run; the shift offsets are sharded across ranks."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--num_inference_steps", type=int, default=50)
    p.add_argument("--shift_steps", type=int, default=16)
    p.add_argument("--output_path", type=str, default="results/shift_ldm.gif")
    p.add_argument("--input_path", type=str, default=None)
    p.add_argument("--ckpt", type=str, default=os.environ.get("AFLDM_CKPT"))
    p.add_argument("--random-init", action="store_true")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--sequential", action="store_true",
                   help="one B = 1 sampler run per offset like the reference loop (default: all offsets of a rank in one batch)")
    p.add_argument("--eager", action="store_true",
                   help="run the STORE / LOAD passes as the eager per-step loop that follows the reference statement by statement "
                        "instead of replayed HIP graphs (afldm_amd.harness.CrossFrameSampler)")
    p.add_argument("--fixed_resize", action="store_true",
                   help="opt OUT of the reference-exact flow: resize --input_path to sample_size x VAE ratio (256) before the VAE "
                        "(the reference resizes to sample_size = 32 and inverts a 4 x 4 latent) and draw the noise on the CPU")
    p.add_argument("--vanilla", action="store_true",
                   help="run the vanilla LDM baseline: skip make_af_unet / make_af_vae_from_config and run the plain strided / "
                        "nearest-neighbour resamplers on HIP (af_api.enable_vanilla_resampling) on both models")
    p.add_argument("--reference_exact", action="store_true", help="accepted for compatibility: this is the default now")
    return p.parse_args()


def main():
    args = parse_args()
    from afldm_amd import compat, parallel
    compat.install()
    from afldm.af_modules.af_api import enable_vanilla_resampling, make_af_unet, make_af_vae_from_config
    from afldm.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.harness import shift_ldm
    rank, world, local = parallel.init_distributed()
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if args.ckpt:
        pipe = MyLDMPipeline.from_pretrained(args.ckpt)
    elif args.random_init:
        import json
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
        pipe = MyLDMPipeline(vae, unet, DDIMScheduler.from_config(FFHQ_DDIM_CONFIG))
    else:
        raise SystemExit("pass --ckpt DIR (or AFLDM_CKPT) or --random-init; checkpoints cannot be downloaded here")
    pipe = pipe.to(f"cuda:{local}").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    if args.vanilla:
        enable_vanilla_resampling(pipe.unet)
        enable_vanilla_resampling(pipe.vae)
    else:
        make_af_unet(pipe.unet)
        make_af_vae_from_config(pipe.vae)
    frames, errs = shift_ldm(pipe, args.num_inference_steps, args.shift_steps, args.output_path, args.input_path,
                             generator=torch.Generator().manual_seed(args.seed), rank=rank, world=world, batch_offsets=not args.sequential,
                             reference_exact=not args.fixed_resize, use_graph=not args.eager)
    if rank == 0:
        print(f"wrote {args.output_path}: {len(frames)} frames; latent equivariance mask-MSE per offset:",
              " ".join(f"{e:.3e}" for e in errs))


if __name__ == "__main__":
    main()
