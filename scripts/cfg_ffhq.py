#!/usr/bin/env python
"""Class-conditional sampling with classifier-free guidance on MI355X - CFG (Ho & Salimans 2022) over class labels on a
class-conditional latent-diffusion UNet of the FFHQ architecture (afldm_amd MyLDMPipeline.cfg: every evaluation runs the UNet on the
conditional rows and, in the same batch, on the unconditional rows, on replayed HIP graphs, and steers away from the second
prediction; decode).  --labels are the class labels, one sample each; --guidance-scale is w in e_c + (w - 1) (e_c - e_u) (1 = the
conditional sampler, no second half); --guidance-rescale pulls the guided prediction's standard deviation back towards the
conditional one's (diffusers' rescale_noise_cfg); --null-label names the row of the embedding table that stands for "no label"
(default: the last one).

No network on the target machines: pass --ckpt /path/to/checkpoint (diffusers-format directory with unet/, scheduler/, vae/, whose
UNet config has num_class_embeds) or --random-init --num-classes K for seeded random weights of the FFHQ architecture with a table of
K classes (demonstrates the full flow; the pictures are noise - there is no class-conditional checkpoint of this model).  Writes one
PNG per sample.

--timings: no picture.  In one process, after a warm-up of each, the latent-space call on replayed graphs at --guidance-scale, the
same at guidance scale 1 (half the UNet rows) and the eager loop, --reps alternated rounds; prints one JSON line with the median
and every run's wall-clock seconds."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--output", type=str, default="results/cfg.png")
    p.add_argument("--labels", type=str, default="0", help="comma-separated class labels, one sample each")
    p.add_argument("--guidance-scale", type=float, default=3.0)
    p.add_argument("--guidance-rescale", type=float, default=0.0)
    p.add_argument("--null-label", type=int, default=None, help="the table row of 'no label' (default: the last one)")
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--seed", type=int, default=1234)
    src = p.add_mutually_exclusive_group()
    src.add_argument("--ckpt", type=str, default=None)
    src.add_argument("--random-init", action="store_true", help="seeded random weights of the FFHQ architecture (needs --num-classes)")
    p.add_argument("--num-classes", type=int, default=None, help="rows of the class table of --random-init, the null class included")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the eager loop instead of replayed HIP graphs")
    p.add_argument("--timings", action="store_true", help="measure instead of writing a picture (see the module docstring)")
    p.add_argument("--reps", type=int, default=3)
    args = p.parse_args(argv)
    if not args.random_init and not args.ckpt:
        args.ckpt = os.environ.get("AFLDM_CKPT")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt DIR or --random-init --num-classes K")
    if args.random_init and (args.num_classes is None or args.num_classes < 2):
        p.error("--random-init needs --num-classes K >= 2 (the last class is the null class)")
    if args.guidance_scale < 1 or not 0 <= args.guidance_rescale <= 1 or args.steps < 1 or args.reps < 1:
        p.error("--guidance-scale must be >= 1, --guidance-rescale in [0, 1], --steps and --reps >= 1")
    try:
        args.labels = [int(s) for s in args.labels.split(",") if s.strip()]
    except ValueError:
        p.error("--labels is a comma-separated list of integers")
    if not args.labels:
        p.error("--labels names no class")
    return args


def build_pipeline(args, with_vae=True):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    if args.ckpt:
        return MyLDMPipeline.from_pretrained(args.ckpt)
    from afldm_amd.configs import FFHQ_DDIM_CONFIG, FFHQ_UNET_CONFIG
    from afldm_amd.models.unet_2d import UNet2DModel
    from afldm_amd.models.vae import AutoencoderKL
    from afldm_amd.schedulers.ddim import DDIMScheduler
    torch.manual_seed(0)
    unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG, num_class_embeds=args.num_classes)
    with torch.no_grad():
        unet.conv_out.weight.mul_(0.1)
        unet.conv_out.bias.mul_(0.1)
    vae = None
    if with_vae:
        vae = AutoencoderKL(in_channels=3, out_channels=3, down_block_types=["DownEncoderBlock2D"] * 4,
                            up_block_types=["UpDecoderBlock2D"] * 4, block_out_channels=[128, 256, 512, 512],
                            layers_per_block=2, latent_channels=4, scaling_factor=0.6, mid_act=True,
                            down_filtered_act=[False, True, True, True], up_filtered_act=[True, True, True, False],
                            up_rescale=[True, True, True])
    return MyLDMPipeline(vae, unet, DDIMScheduler.from_config(FFHQ_DDIM_CONFIG))


def timings(args, pipe):
    c, s = pipe.unet.config.in_channels, pipe.unet.config.sample_size
    x = torch.randn(len(args.labels), c, s, s, generator=torch.Generator().manual_seed(args.seed))
    kw = dict(class_labels=args.labels, guidance_rescale=args.guidance_rescale, null_label=args.null_label, eta=args.eta,
              num_inference_steps=args.steps, latents=x)

    def own():          # a pipeline keeps ONE engine per sampler: one pipeline per setting
        q = type(pipe)(None, pipe.unet, pipe.scheduler)
        q.set_progress_bar_config(disable=True)
        return q
    guided, plain, eager = own(), own(), own()
    runs = {"graph": lambda: guided.cfg_latents(guidance_scale=args.guidance_scale, generator=torch.Generator().manual_seed(1), **kw),
            "graph_scale_1": lambda: plain.cfg_latents(guidance_scale=1.0, generator=torch.Generator().manual_seed(1), **kw),
            "eager": lambda: eager.cfg_latents(guidance_scale=args.guidance_scale, generator=torch.Generator().manual_seed(1),
                                               use_graph=False, **kw)}
    wall = {k: [] for k in runs}
    for fn in runs.values():          # warm-up: capture, packing, workspaces
        fn()
        torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
    out = {"what": "cfg", "dtype": args.dtype, "batch": len(args.labels), "steps": args.steps, "guidance_scale": args.guidance_scale,
           "guidance_rescale": args.guidance_rescale, "eta": args.eta, "reps": args.reps, "random_weights": bool(args.random_init)}
    for k, ts in wall.items():
        out[k + "_s"] = round(statistics.median(ts), 4)
        out[k + "_runs_s"] = [round(t, 4) for t in ts]
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args, with_vae=not args.timings).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    if pipe.vae is not None:
        make_af_vae_from_config(pipe.vae)
    if args.timings:
        return timings(args, pipe)
    out = pipe.cfg(args.labels, guidance_scale=args.guidance_scale, guidance_rescale=args.guidance_rescale, null_label=args.null_label,
                   eta=args.eta, num_inference_steps=args.steps, generator=torch.Generator().manual_seed(args.seed),
                   use_graph=not args.eager, output_type="pil")
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    stem, ext = os.path.splitext(args.output)
    for i, im in enumerate(out.images):
        im.save(args.output if len(out.images) == 1 else f"{stem}_{i}{ext}")
    null = pipe.unet.config.num_class_embeds - 1 if args.null_label is None else args.null_label
    print(f"wrote {len(out.images)} image(s) to {args.output}: labels {args.labels}, guidance_scale {args.guidance_scale}, "
          f"guidance_rescale {args.guidance_rescale}, null label {null}")
    return out.images


if __name__ == "__main__":
    main()
