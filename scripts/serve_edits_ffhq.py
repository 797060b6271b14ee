#!/usr/bin/env python
"""FFHQ edits served in slots on MI355X - continuous batching of image-conditioned requests (afldm_amd.serving.SamplingServer with
the "seeded_sdedit" and "seeded_repaint" kinds): img2img requests of different strengths, RePaint inpainting requests and
unconditional samples share the batch-`--slots` replayed HIP graphs, and a slot that finishes takes the next request while its
neighbours go on.  Every noise of an edit is a function of its seed, so a request gives the same picture whatever it is served with.

  --requests 9         request i is: i % 3 == 0 an img2img edit of strength --strengths[i // 3 % len], i % 3 == 1 an inpainting
                       request (the mask's black part is generated), i % 3 == 2 an unconditional sample of --steps steps
  --strengths 0.3,0.6  img2img strengths, cycled
  --slots 4            batch rows of the replayed graph

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/, scheduler/,
vae/) with --input_path / --mask_path, or --random-init for seeded random weights of the FFHQ architecture and a synthetic image
and mask (demonstrates the full flow; the pictures are noise).  Writes one PNG per request."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from inpaint_ffhq import build_pipeline, load_mask, synthetic_inputs  # noqa: E402  (the same pipeline sources and inputs)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--output", type=str, default="results/edits.png")
    p.add_argument("--input_path", type=str, default=None)
    p.add_argument("--mask_path", type=str, default=None, help="white = keep, black = generate (img2img: black = change value 1)")
    p.add_argument("--requests", type=int, default=9)
    p.add_argument("--slots", type=int, default=4)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--strengths", type=str, default="0.3,0.6", help="comma-separated img2img strengths, cycled")
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--inpaint-steps", type=int, default=20)
    p.add_argument("--jump-length", type=int, default=5)
    p.add_argument("--jump-n-sample", type=int, default=2)
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
    if not args.random_init and not (args.input_path and args.mask_path):
        p.error("pass --input_path and --mask_path (or --random-init for a synthetic image and mask)")
    args.strengths = [float(s) for s in args.strengths.split(",") if s.strip()]
    if not args.strengths or args.requests < 1 or args.slots < 1 or args.steps < 1:
        p.error("--strengths, --requests, --slots and --steps must be given and >= 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    from afldm_amd.io_utils import image_to_tensor
    from afldm_amd.serving import SamplingServer
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
        mask = load_mask(args.mask_path, size)
    server = SamplingServer(pipe, args.slots, kinds=("ddim", "seeded", "seeded_sdedit", "seeded_repaint"))
    tickets, names = [], []
    for i in range(args.requests):
        seed = args.seed + i
        if i % 3 == 0:
            strength = args.strengths[i // 3 % len(args.strengths)]
            tickets.append(server.submit_img2img(image, strength, 1.0 - mask, args.steps, args.eta, seed=seed))
            names.append(f"img2img {strength}")
        elif i % 3 == 1:
            tickets.append(server.submit_inpaint(image, mask, args.inpaint_steps, args.eta, args.jump_length, args.jump_n_sample,
                                                 seed=seed))
            names.append("inpaint")
        else:
            tickets.append(server.submit(args.steps, seed=seed))
            names.append("sample")
    server.run()
    out = server.decode(tickets, output_type="pil")
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    stem, ext = os.path.splitext(args.output)
    for i, im in enumerate(out.images):
        im.save(args.output if len(out.images) == 1 else f"{stem}_{i}{ext}")
    counts = [t.steps for t in tickets]
    print(f"wrote {len(out.images)} image(s) to {args.output}: {', '.join(names)} with {counts} evaluations on {args.slots} slots, "
          f"{server.replays} graph replays, {server.useful} of {server.evaluations} slot evaluations useful")
    return out.images


if __name__ == "__main__":
    main()
