#!/usr/bin/env python
"""FFHQ outpainting on MI355X - RePaint (Lugmayr et al., CVPR 2022) on a MultiDiffusion canvas (Bar-Tal et al., ICML 2023) with the
unconditional FFHQ latent-diffusion model (afldm_amd MyLDMPipeline.outpaint): a 256 x 256 image is encoded, pasted into a larger
latent canvas and the picture around it sampled through overlapping windows, every UNet evaluation ending in one fused
afldm_pano_repaint_step on replayed HIP graphs; then the canvas is decoded window by window and the input's pixels pasted back.
--width / --height / --left / --top / --stride are in PIXELS (multiples of the VAE's scale factor 8; the image is centred by
default, the stride defaults to a quarter window); --circular wraps the x axis, and the paste with it.

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) and --image, or --random-init for seeded random weights of the FFHQ architecture and a seeded synthetic image
(demonstrates the full flow; the picture is noise).  Writes one PNG.

--timings: no picture.  afldm_pano_repaint_step and afldm_pano_step on the same canvas are each captured `--launches` times into
one graph and the replays alternate between device events `--reps` times.  Prints one JSON line with the medians and every run."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))          # (the sibling scripts: the pipeline and the synthetic image)
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--image", type=str, default=None, help="the picture to keep (resized to the model's 256 x 256)")
    p.add_argument("--out", "--output", dest="out", type=str, default="results/outpaint.png")
    p.add_argument("--width", type=int, default=768, help="pixels")
    p.add_argument("--height", type=int, default=256, help="pixels")
    p.add_argument("--left", type=int, default=None, help="pixels from the canvas's left edge to the image's (default: centred)")
    p.add_argument("--top", type=int, default=None, help="pixels from the canvas's top edge to the image's (default: centred)")
    p.add_argument("--keep-margin", type=int, default=0, help="latents at the image's border handed to the sampler")
    p.add_argument("--stride", type=int, default=None, help="pixels between windows (default: a quarter window)")
    p.add_argument("--circular", action="store_true", help="wrap the x axis")
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--jump_length", type=int, default=10)
    p.add_argument("--jump_n_sample", type=int, default=10)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--no-composite", action="store_true", help="write the decoded canvas itself instead of pasting the kept pixels")
    src = p.add_mutually_exclusive_group()
    src.add_argument("--ckpt", type=str, default=None)
    src.add_argument("--random-init", action="store_true",
                     help="seeded random weights of the FFHQ architecture and a synthetic image")
    p.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the eager loop instead of replayed HIP graphs")
    p.add_argument("--timings", action="store_true", help="measure the update kernel instead of writing a picture")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--launches", type=int, default=200)
    args = p.parse_args(argv)
    if not args.random_init and not args.ckpt:
        args.ckpt = os.environ.get("AFLDM_CKPT")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt DIR or --random-init")
    if not args.random_init and not args.image and not args.timings:
        p.error("pass --image (or --random-init for a synthetic one)")
    if min(args.steps, args.jump_length, args.jump_n_sample, args.reps, args.launches) < 1:
        p.error("--steps, --jump_length, --jump_n_sample, --reps and --launches must be >= 1")
    return args


def timings(args, pipe, h, w, stride):
    """The two canvas updates, graph-replayed: `launches` dependent updates per replay, the gaps between them included."""
    from afldm_amd import ops
    geom = pipe.panorama_geometry(h, w, stride, args.circular)
    n, c, s = geom.nwin, pipe.unet.config.in_channels, pipe.unet.config.sample_size
    g = torch.Generator("cuda").manual_seed(n)
    eps = torch.randn(n, s, s, c, device="cuda", generator=g).to(pipe.unet.dtype)
    x0 = torch.randn(1, c, h, w, device="cuda", generator=g)
    known = torch.randn(1, c, h, w, device="cuda", generator=g)
    mask = torch.zeros(1, 1, h, w, device="cuda")
    mask[..., (w - s) // 2:(w + s) // 2] = 1.0
    inf = float("inf")
    pano = torch.tensor((1.0, -0.5, -inf, inf, 0.0, 0.83, 0.28, 0.49), dtype=torch.float32, device="cuda")    # chained: stays finite
    rep = torch.tensor((1.0, -0.5, -inf, inf, 0.83, 0.28, 0.49, 0.8, 0.6, 0.9, 0.43, 0.0), dtype=torch.float32, device="cuda")
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    nz1, nz3 = torch.randn(1, 1, c, h, w, device="cuda", generator=g), torch.randn(1, 3, 1, c, h, w, device="cuda", generator=g)
    ones, x, y = torch.ones(s, s, device="cuda"), x0.clone(), x0.clone()
    win = torch.empty(n, c, s, s, device="cuda")
    loops = {"pano_repaint_step_us": (lambda: ops.pano_repaint_step(x, eps, known, mask, nz3, ones, geom, rep, zero, out=x,
                                                                    windows_out=win), x),
             "pano_step_us": (lambda: ops.pano_step(y, eps, nz1, ones, geom, pano, zero, out=y, windows_out=win), y)}
    graphs = {}
    for k, (fn, buf) in loops.items():
        fn()
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(args.launches):
                fn()
    kern = {k: [] for k in loops}
    for i in range(args.reps + 1):
        for k, (fn, buf) in loops.items():
            buf.copy_(x0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[k].replay()
            e1.record()
            torch.cuda.synchronize()
            if i:
                kern[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    out = {"what": "outpaint", "dtype": args.dtype, "canvas_latents": [h, w], "circular": args.circular, "nwin": n,
           "reps": args.reps, "launches_per_replay": args.launches}
    for k, ts in kern.items():
        out[k] = round(statistics.median(ts), 2)
        out[k[:-3] + "_runs_us"] = [round(t, 2) for t in ts]
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    args = parse_args(argv)
    from inpaint_ffhq import synthetic_inputs
    from panorama_ffhq import build_pipeline
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args, with_vae=not args.timings).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    r = 8
    if pipe.vae is not None:
        make_af_vae_from_config(pipe.vae)
        r = 2 ** (len(pipe.vae.config.block_out_channels) - 1)
    for name in ("width", "height", "stride", "left", "top"):
        v = getattr(args, name)
        if v is not None and (v % r or v < (0 if name in ("left", "top") else r)):
            raise SystemExit(f"--{name} {v} must be a multiple of {r} pixels")
    if args.timings:
        return timings(args, pipe, args.height // r, args.width // r, None if args.stride is None else args.stride // r)
    size = pipe.unet.config.sample_size * r
    if args.image:
        from afldm_amd.io_utils import image_to_tensor
        image = image_to_tensor(args.image, resolution=(size, size))
    else:
        image = synthetic_inputs(args.seed, size)[0]
    out = pipe.outpaint(image, args.height, args.width, top=args.top, left=args.left, keep_margin=args.keep_margin,
                        stride=args.stride, circular=args.circular, num_inference_steps=args.steps, eta=args.eta,
                        jump_length=args.jump_length, jump_n_sample=args.jump_n_sample,
                        generator=torch.Generator().manual_seed(args.seed), use_graph=not args.eager,
                        composite=not args.no_composite, output_type="pil")
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    out.images[0].save(args.out)
    print(f"wrote {args.out}: {args.width} x {args.height} around a {size} x {size} image"
          f"{', circular' if args.circular else ''}, eta {args.eta}, {args.steps} steps")
    return out.images[0]


if __name__ == "__main__":
    main()
