#!/usr/bin/env python
"""Flow-guided interpolation on MI355X, reported, not gated:
  1. the noise warp of a 17-frame warp_method=0 call: 15 intermediate frames x 2 endpoints, 4 channels, 32^2 -> 256^2, fp32.
     Batched: per endpoint one ideal up-sampling and ONE pick-mode afldm_flow_splat call over all frames (only the kept
     targets accumulated, the fill read in place).  Per frame, unfused, with the same ops: up-sample once per endpoint, then
     per frame a full-resolution splat, the fill expression and the [::8, ::8] slice in torch.  Both as HIP-graph time (20 calls
     per graph) and as eager wall time (launch + Python overhead included, which is what a pipeline call pays);
  2. a whole 17-frame, 50-step LDMInterpolationPipeline call (FFHQ-size UNet + AF-VAE, seeded random weights, bf16) with
     warp_method=0 and a smooth synthetic flow pair against warp_method=3 on the same images (graph path, replays)."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402


def smooth_flows(S, A):
    """(fwd, bwd) [1, 2, S, S], channel 0 = x: a smooth field of amplitude A pixels and its negative."""
    i, j = torch.meshgrid(torch.arange(S, dtype=torch.float64), torch.arange(S, dtype=torch.float64), indexing="ij")
    rows = -A * torch.sin(2 * math.pi * (i / S + 0.3 * j / S) + 0.4)
    cols = -A * torch.cos(2 * math.pi * (j / S - 0.2 * i / S) + 1.1)
    f = torch.stack([cols, rows])[None].float().cuda()
    return f, -f


def wall(fn, iters=20):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def warp(frames=17, C=4, h=32, ds=8):
    from afldm_amd import ops
    from afldm_amd.af_libs.ideal_lpf import UpsampleRFFT
    from afldm_amd.shift_utils import flow_utils as fu
    from bench_kernels import timeit_graph
    S, n = h * ds, frames - 2
    g = torch.Generator().manual_seed(0)
    z = [torch.randn(1, C, h, h, generator=g).cuda() for _ in range(2)]
    flows = [torch.flip(f, (1,)).contiguous() for f in smooth_flows(S, 12.0)]
    bg = torch.randn(1, C, S, S, generator=g).cuda()
    alphas = torch.linspace(0, 1, frames)
    sc = [alphas[1:-1].cuda().contiguous(), (1 - alphas)[1:-1].cuda().contiguous()]
    one = [[s[i:i + 1].contiguous() for i in range(n)] for s in sc]
    up = UpsampleRFFT(ds)

    def batched():
        return [fu.forward_flow_warp_frames(up(z[e]), flows[e], sc[e], ds=ds, fill=bg)[0] for e in range(2)]

    def per_frame():
        out = []
        for e in range(2):
            hi = up(z[e])
            for i in range(n):
                res, occ = ops.flow_splat(hi, flows[e], one[e][i])
                out.append((res * (1 - occ) + occ * bg)[:, :, ::ds, ::ds])
        return out

    def splat_only():
        return [ops.flow_splat(hi[e], flows[e], sc[e], ds=ds, fill=bg, fill_pix_stride=ds) for e in range(2)]
    hi = [up(v) for v in z]
    a, b = batched(), per_frame()
    diff = max(float((a[e][i] - b[e * n + i][0]).abs().max()) for e in range(2) for i in range(n))
    print(f"== noise warp: {n} frames x 2 endpoints, {C} channels, {h}^2 -> {S}^2, fp32 (max |batched - per frame| {diff:.2e})",
          flush=True)
    tg_b, tg_p, tg_s = timeit_graph(batched), timeit_graph(per_frame, reps=4), timeit_graph(splat_only)
    tw_b, tw_p = wall(batched), wall(per_frame, iters=5)
    print(f"HIP graph: batched {tg_b:8.1f} us (of which the two splat calls {tg_s:.1f}) | per frame, unfused {tg_p:8.1f} us "
          f"({tg_p / tg_b:.1f}x)", flush=True)
    print(f"eager    : batched {tw_b:8.1f} us | per frame, unfused {tw_p:8.1f} us ({tw_p / tw_b:.1f}x)", flush=True)


def whole_call(frames=17, steps=50, dtype=torch.bfloat16):
    import image_interpolation_ffhq as script
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    args = script.parse_args(["--random-init"])
    pipe = script.build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    images = script.synthetic_images(1234)
    flows = smooth_flows(pipe.unet.config.sample_size * pipe.vae_scale_factor, 12.0)
    print(f"== whole call: {frames} frames, {steps} DDIM steps, FFHQ-size UNet + AF-VAE, {dtype}, output_type='pt', graph path",
          flush=True)
    for name, kw in (("warp_method=3, first call (captures)", {}), ("warp_method=3, replay", {}), ("warp_method=3, replay", {}),
                     ("warp_method=0, replay", dict(warp_method=0, flows=flows)),
                     ("warp_method=0, replay", dict(warp_method=0, flows=flows)),
                     ("warp_method=1, replay", dict(warp_method=1, flows=flows)),
                     ("warp_method=2, replay", dict(warp_method=2, flows=flows))):
        tm = {}
        if "flows" in kw:
            kw["generator"] = torch.Generator().manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(*images, num_frames=frames, num_inference_steps=steps, output_type="pt", timings=tm, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        parts = ", ".join(f"{k} {v:.3f}" for k, v in sorted(tm.items()) if k != "total_s")
        print(f"{name:38s} {dt:8.3f} s  ({parts})", flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=17)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warp-only", action="store_true")
    a = p.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    warp(a.frames)
    if not a.warp_only:
        whole_call(a.frames, a.steps)
