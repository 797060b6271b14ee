#!/usr/bin/env python
"""FFHQ at twice the resolution on MI355X - high-resolution sampling after DemoFusion (Du et al., CVPR 2024) on the unconditional
FFHQ latent-diffusion model (afldm_amd MyLDMPipeline.hires): a base sample at the model's own 256 x 256, its latents upsampled and
re-noised, and the canvas of --scale times the window denoised through MultiDiffusion windows plus a skip residual towards the
noised reference and --scale^2 dilated windows behind the ideal low-pass of cut-off 1 / scale - every UNet evaluation ending in one
fused afldm_hires_step on replayed HIP graphs - then decoded window by window and blended under a triangular feather.  --stride is
in PIXELS (a multiple of the VAE's scale factor 8; default half a window).  The canvas is at most 64 x 64 latents: --scale 2.

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture (demonstrates the full flow; the picture
is noise).  Writes one PNG.

--timings: no picture.  In one process, after a warm-up of each, the latent-space hires call on replayed graphs, its eager loop
and the plain sampler (MyLDMPipeline.__call__) at a batch of as many planes as the canvas has windows ALTERNATE `--reps` times,
each run ended by a device synchronise; then afldm_hires_step and afldm_pano_repaint_step on the same canvas and local windows are
each captured `--launches` times into one graph and the replays alternate between device events.  Prints one JSON line with the
medians, every run and a fingerprint of the box."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", "--output", dest="out", type=str, default="results/hires.png")
    p.add_argument("--scale", type=int, default=2, help="the canvas is scale x the model's window per axis")
    p.add_argument("--stride", type=int, default=None, help="pixels between local windows (default: half a window)")
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--cosine-scale-1", type=float, default=3.0, help="skip residual; negative: off")
    p.add_argument("--cosine-scale-2", type=float, default=1.0, help="dilated sampling; negative: off")
    p.add_argument("--cosine-scale-3", type=float, default=1.0, help="low-pass of the dilated views; negative: off")
    p.add_argument("--seed", type=int, default=1234)
    src = p.add_mutually_exclusive_group()
    src.add_argument("--ckpt", type=str, default=None)
    src.add_argument("--random-init", action="store_true", help="seeded random weights of the FFHQ architecture")
    p.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    p.add_argument("--eager", action="store_true", help="run the eager loop instead of replayed HIP graphs")
    p.add_argument("--timings", action="store_true", help="measure instead of writing a picture (see the module docstring)")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--launches", type=int, default=200)
    args = p.parse_args(argv)
    if not args.random_init and not args.ckpt:
        args.ckpt = os.environ.get("AFLDM_CKPT")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt DIR or --random-init")
    if args.steps < 1 or args.reps < 1 or args.launches < 1 or args.scale < 2:
        p.error("--steps, --reps and --launches must be >= 1 and --scale >= 2")
    for k in ("cosine_scale_1", "cosine_scale_2", "cosine_scale_3"):
        if getattr(args, k) < 0:
            setattr(args, k, None)
    return args


def timings(args, pipe, stride):
    from afldm_amd import ops
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    from panorama_ffhq import box_fingerprint
    scale, c, s = args.scale, pipe.unet.config.in_channels, pipe.unet.config.sample_size
    h = scale * s
    geom = pipe.panorama_geometry(h, h, s // 2 if stride is None else stride)
    n, NW = geom.nwin, geom.nwin + scale * scale
    base = torch.randn(1, c, s, s, generator=torch.Generator().manual_seed(args.seed))
    plain = torch.randn(NW, c, s, s, generator=torch.Generator().manual_seed(args.seed))
    kw = dict(scale=scale, stride=stride, eta=args.eta, num_inference_steps=args.steps, cosine_scale_1=args.cosine_scale_1,
              cosine_scale_2=args.cosine_scale_2, cosine_scale_3=args.cosine_scale_3)

    def hires(use_graph):
        return pipe.hires_latents(base, generator=torch.Generator().manual_seed(1), use_graph=use_graph, **kw)

    runs = {"hires_graph": lambda: hires(True),
            "hires_eager": lambda: hires(False),
            "sampler_batch_nw_graph": lambda: pipe(latents=plain, eta=args.eta, num_inference_steps=args.steps, output_type="latent",
                                                   generator=torch.Generator().manual_seed(1))}
    wall = {k: [] for k in runs}
    for k, fn in runs.items():                                             # warm-up: capture, packing, workspaces
        fn()
        torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
    # the two update launches, graph-replayed: `launches` dependent updates per replay, the gaps between them included
    dtype = pipe.unet.dtype
    g = torch.Generator("cuda").manual_seed(n)

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=g)
    eps, x0, ref, eps_ref, nz = rn(NW, s, s, c).to(dtype), rn(1, c, h, h), rn(1, c, h, h), rn(1, c, h, h), rn(1, 3, 1, c, h, h)
    # |a p| < 1: chained updates stay finite.  "hires": every term on; "repaint": a soft mask and all three slots live
    inf = float("inf")
    hrow = torch.tensor((1.0, -0.5, -inf, inf, 0.83, 0.28, 0.49, 0.8, 0.6, 0.3, 0.5, 0.5), dtype=torch.float32, device="cuda")
    rrow = torch.tensor((1.0, -0.5, -inf, inf, 0.83, 0.28, 0.49, 0.8, 0.6, 0.9, 0.43, 0.0), dtype=torch.float32, device="cuda")
    mask = torch.rand(1, 1, h, h, device="cuda", generator=g)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = ilvr_filter(h, scale).to(device="cuda", dtype=torch.float32).contiguous()
    ones, x, y = torch.ones(s, s, device="cuda"), x0.clone(), x0.clone()
    win_h, win_r = torch.empty(NW, c, s, s, device="cuda"), torch.empty(n, c, s, s, device="cuda")
    loops = {"hires_step_us": (lambda: ops.hires_step(x, eps, ref, eps_ref, nz[:, 1], ones, L, L, geom, scale, hrow, zero, out=x,
                                                      windows_out=win_h), x),
             "pano_repaint_step_us": (lambda: ops.pano_repaint_step(y, eps[:n], ref, mask, nz, ones, geom, rrow, zero, out=y,
                                                                    windows_out=win_r), y)}
    graphs = {}
    for k, (fn, buf) in loops.items():
        fn()
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(args.launches):
                fn()
    kern = {k: [] for k in loops}
    for rep in range(args.reps + 1):
        for k, (fn, buf) in loops.items():
            buf.copy_(x0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[k].replay()
            e1.record()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(buf).all()), k
            if rep:
                kern[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    out = {"what": "hires", "dtype": args.dtype, "canvas_latents": [h, h], "scale": scale,
           "stride_latents": geom.ox[1] if geom.nx > 1 else None, "local_windows": n, "windows": NW, "steps": args.steps,
           "eta": args.eta, "cosine_scales": [args.cosine_scale_1, args.cosine_scale_2, args.cosine_scale_3], "reps": args.reps,
           "launches_per_replay": args.launches}
    for k, ts in wall.items():
        out[k + "_s"] = round(statistics.median(ts), 4)
        out[k + "_ms_per_evaluation"] = round(statistics.median(ts) / args.steps * 1e3, 3)
        out[k + "_runs_s"] = [round(t, 4) for t in ts]
    out["pair_differences_ms_per_evaluation"] = [round((a - b) / args.steps * 1e3, 3)
                                                 for a, b in zip(wall["hires_graph"], wall["sampler_batch_nw_graph"])]
    for k, ts in kern.items():
        out[k] = round(statistics.median(ts), 2)
        out[k[:-3] + "_runs_us"] = [round(t, 2) for t in ts]
    out["box"] = box_fingerprint()
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    from panorama_ffhq import build_pipeline
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args, with_vae=not args.timings).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    r = 8
    if pipe.vae is not None:
        make_af_vae_from_config(pipe.vae)
        r = 2 ** (len(pipe.vae.config.block_out_channels) - 1)
    if args.stride is not None and (args.stride % r or args.stride < r):
        raise SystemExit(f"--stride {args.stride} must be a positive multiple of {r} pixels")
    if args.timings:
        return timings(args, pipe, None if args.stride is None else args.stride // r)
    out = pipe.hires(1, args.scale, stride=args.stride, eta=args.eta, num_inference_steps=args.steps,
                     cosine_scale_1=args.cosine_scale_1, cosine_scale_2=args.cosine_scale_2, cosine_scale_3=args.cosine_scale_3,
                     generator=torch.Generator().manual_seed(args.seed), use_graph=not args.eager, output_type="pil")
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    out.images[0].save(args.out)
    side = args.scale * pipe.unet.config.sample_size * r
    print(f"wrote {args.out}: {side} x {side}, scale {args.scale}, stride {args.stride or 'half a window'}, eta {args.eta}, "
          f"{args.steps} steps")
    return out.images[0]


if __name__ == "__main__":
    main()
