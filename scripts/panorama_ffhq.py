#!/usr/bin/env python
"""FFHQ panoramas on MI355X - MultiDiffusion (Bar-Tal et al., ICML 2023) on the unconditional FFHQ latent-diffusion model
(afldm_amd MyLDMPipeline.panorama): a canvas wider (and / or taller) than the 256 x 256 window the model was trained on is
sampled through overlapping windows, every UNet evaluation ending in one fused afldm_pano_step on replayed HIP graphs, then decoded
window by window and blended under a triangular feather.  --width / --height / --stride are in PIXELS (multiples of the VAE's
scale factor 8; the stride defaults to a quarter window); --circular wraps the x axis (a seamless 360-degree strip).

No network on the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/,
scheduler/, vae/) or --random-init for seeded random weights of the FFHQ architecture (demonstrates the full flow; the picture
is noise).  Writes one PNG.

--timings: no picture.  In one process, after a warm-up of each, the latent-space panorama call on replayed graphs, the plain
sampler (MyLDMPipeline.__call__) at batch nwin and the panorama's eager loop ALTERNATE `--reps` times, each run ended by a device
synchronise; then afldm_pano_step and afldm_sde_step at batch nwin are each captured `--launches` times into one graph and the
replays alternate between device events.  Prints one JSON line with the medians, every run and a fingerprint of the box."""
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
    p.add_argument("--out", "--output", dest="out", type=str, default="results/panorama.png")
    p.add_argument("--width", type=int, default=1024, help="pixels")
    p.add_argument("--height", type=int, default=256, help="pixels")
    p.add_argument("--stride", type=int, default=None, help="pixels between windows (default: a quarter window)")
    p.add_argument("--circular", action="store_true", help="wrap the x axis")
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--steps", type=int, default=50)
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
    if args.steps < 1 or args.reps < 1 or args.launches < 1:
        p.error("--steps, --reps and --launches must be >= 1")
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
    unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG)
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


def box_fingerprint():
    """What tells one MI355X box from another in a latency-bound measurement: the device, a 256 MiB device-to-device copy and the
    boundary between two dependent empty kernels of a replayed graph."""
    from afldm_amd import _lib
    props = torch.cuda.get_device_properties(0)
    st = lambda: torch.cuda.current_stream().cuda_stream           # noqa: E731

    def timed(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)
    nbytes = 256 << 20
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 255)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: _lib.check(_lib.lib.afldm_probe_copy(src.data_ptr(), dst.data_ptr(), nbytes, st()), "probe_copy"))
    empty = lambda: _lib.check(_lib.lib.afldm_probe_empty(props.multi_processor_count, st()), "probe_empty")      # noqa: E731
    empty()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(200):
            empty()
    empty_ms = timed(g.replay)
    return {"device": props.name, "cus": props.multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip,
            "copy_gbs": round(2 * nbytes / copy_ms / 1e6, 1), "empty_kernel_boundary_us": round(empty_ms * 1e3 / 200, 2)}


def timings(args, pipe, h, w, stride):
    from afldm_amd import ops
    geom = pipe.panorama_geometry(h, w, stride, args.circular)
    n, c, s = geom.nwin, pipe.unet.config.in_channels, pipe.unet.config.sample_size
    canvas = torch.randn(1, c, h, w, generator=torch.Generator().manual_seed(args.seed))
    plain = torch.randn(n, c, s, s, generator=torch.Generator().manual_seed(args.seed))
    kw = dict(stride=stride, circular=args.circular, eta=args.eta, num_inference_steps=args.steps, latents=canvas)

    def pano(use_graph):
        return pipe.panorama_latents(h, w, generator=torch.Generator().manual_seed(1), use_graph=use_graph, **kw)

    runs = {"panorama_graph": lambda: pano(True),
            "sampler_batch_nwin_graph": lambda: pipe(latents=plain, eta=args.eta, num_inference_steps=args.steps, output_type="latent",
                                                     generator=torch.Generator().manual_seed(1)),
            "panorama_eager": lambda: pano(False)}
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
    eps = torch.randn(n, s, s, c, device="cuda", generator=g).to(dtype)
    x0 = torch.randn(1, c, h, w, device="cuda", generator=g)
    y0 = torch.randn(n, c, s, s, device="cuda", generator=g)
    row = (1.0, -0.5, -float("inf"), float("inf"), 0.0, 0.83, 0.28, 0.49)             # |a + b p| < 1: chained updates stay finite
    coef = torch.tensor(row, dtype=torch.float32, device="cuda")
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    nz_c, nz_w = torch.randn(1, 1, c, h, w, device="cuda", generator=g), torch.randn(1, n, c, s, s, device="cuda", generator=g)
    ones, x, y = torch.ones(s, s, device="cuda"), x0.clone(), y0.clone()
    win = torch.empty(n, c, s, s, device="cuda")
    loops = {"pano_step_us": (lambda: ops.pano_step(x, eps, nz_c, ones, geom, coef, zero, out=x, windows_out=win), x, x0),
             "sde_step_batch_nwin_us": (lambda: ops.sde_step(y, eps, nz_w, coef, zero, out=y), y, y0)}
    graphs = {}
    for k, (fn, buf, init) in loops.items():
        fn()
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(args.launches):
                fn()
    kern = {k: [] for k in loops}
    for rep in range(args.reps + 1):
        for k, (fn, buf, init) in loops.items():
            buf.copy_(init)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[k].replay()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                kern[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    out = {"what": "panorama", "dtype": args.dtype, "canvas_latents": [h, w], "stride_latents": geom.ox[1] if geom.nx > 1 else None,
           "circular": args.circular, "nwin": n, "steps": args.steps, "eta": args.eta, "reps": args.reps,
           "launches_per_replay": args.launches}
    for k, ts in wall.items():
        out[k + "_s"] = round(statistics.median(ts), 4)
        out[k + "_ms_per_evaluation"] = round(statistics.median(ts) / args.steps * 1e3, 3)
        out[k + "_runs_s"] = [round(t, 4) for t in ts]
    out["pair_differences_ms_per_evaluation"] = [round((a - b) / args.steps * 1e3, 3)
                                                 for a, b in zip(wall["panorama_graph"], wall["sampler_batch_nwin_graph"])]
    for k, ts in kern.items():
        out[k] = round(statistics.median(ts), 2)
        out[k[:-3] + "_runs_us"] = [round(t, 2) for t in ts]
    out["box"] = box_fingerprint()
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args, with_vae=not args.timings).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    r = 8
    if pipe.vae is not None:
        make_af_vae_from_config(pipe.vae)
        r = 2 ** (len(pipe.vae.config.block_out_channels) - 1)
    for name in ("width", "height", "stride"):
        v = getattr(args, name)
        if v is not None and (v % r or v < r):
            raise SystemExit(f"--{name} {v} must be a positive multiple of {r} pixels")
    if args.timings:
        return timings(args, pipe, args.height // r, args.width // r, None if args.stride is None else args.stride // r)
    out = pipe.panorama(args.height, args.width, stride=args.stride, circular=args.circular, eta=args.eta,
                        num_inference_steps=args.steps, generator=torch.Generator().manual_seed(args.seed),
                        use_graph=not args.eager, output_type="pil")
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    out.images[0].save(args.out)
    print(f"wrote {args.out}: {args.width} x {args.height}, stride {args.stride or 'a quarter window'}"
          f"{', circular' if args.circular else ''}, eta {args.eta}, {args.steps} steps")
    return out.images[0]


if __name__ == "__main__":
    main()
