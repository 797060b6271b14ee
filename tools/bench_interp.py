#!/usr/bin/env python
"""Image interpolation on MI355X:
  1. afldm_attention_interp (one launch, both sources, per-sample alpha) against two afldm_attention launches + the torch blend
     (1 - alpha) o0 + alpha o1, and against ONE single-source launch, at every FFHQ attention level, batch 17, bf16 (HIP-graph
     timing: 20 calls per graph, us per call);
  2. a whole 17-frame, 50-step LDMInterpolationPipeline call (FFHQ-size UNet + AF-VAE, seeded random weights, bf16): the graph
     path (first call = capture, then replays) against use_graph=False (the reference's loop statement by statement)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

LEVELS = [("32^2", 1024, 192, 8), ("16^2", 256, 384, 16), ("8^2", 64, 384, 16), ("4^2", 16, 768, 32), ("2^2", 4, 768, 32)]


def kernels(B=17, dtype=torch.bfloat16):
    from afldm_amd import ops
    from bench_kernels import timeit_graph
    print(f"== kernel: batch {B}, {dtype}, one stored sample per source (Bk = 1), us per call", flush=True)
    for name, T, C, heads in LEVELS:
        g = torch.Generator().manual_seed(T)
        q = torch.randn(B, T, C, generator=g).to(device="cuda", dtype=dtype)
        kb = [torch.randn(1, T, 2 * C, generator=g).to(device="cuda", dtype=dtype) for _ in range(2)]
        k0, k1 = kb[0][:, :, C:], kb[1][:, :, C:]
        vt0, vt1 = (torch.randn(1, C, T, generator=g).to(device="cuda", dtype=dtype) for _ in range(2))
        alpha = torch.linspace(0, 1, B, device="cuda")
        a3 = alpha.view(B, 1, 1).to(dtype)
        out = torch.empty(B, T, C, device="cuda", dtype=dtype)

        def two():
            o0 = ops.attention(q, k0, vt0, heads)
            o1 = ops.attention(q, k1, vt1, heads)
            return (1 - a3) * o0 + a3 * o1
        t_one = timeit_graph(lambda: ops.attention(q, k0, vt0, heads, out=out))
        t_two = timeit_graph(two)
        t_new = timeit_graph(lambda: ops.attention_interp(q, k0, vt0, k1, vt1, alpha, heads, out=out))
        print(f"{name:5s} T={T:4d} C={C:3d} heads={heads:2d}: interp {t_new:7.1f} | 2 x attention + blend {t_two:7.1f} "
              f"| 1 x attention {t_one:7.1f}  (interp / two-launch {t_new / t_two:.2f}, interp / single {t_new / t_one:.2f})",
              flush=True)


def whole_call(frames=17, steps=50, dtype=torch.bfloat16, eager=True):
    import image_interpolation_ffhq as script
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    args = script.parse_args(["--random-init"])
    pipe = script.build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    images = script.synthetic_images(1234)
    print(f"== whole call: {frames} frames, {steps} DDIM steps, FFHQ-size UNet + AF-VAE, {dtype}, output_type='pt'", flush=True)
    runs = [("graph, first call (captures)", True), ("graph, replay", True), ("graph, replay", True)]
    if eager:
        runs.append(("use_graph=False", False))
    for name, graph in runs:
        tm = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(*images, num_frames=frames, num_inference_steps=steps, output_type="pt", use_graph=graph, timings=tm)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        parts = ", ".join(f"{k} {v:.3f}" for k, v in sorted(tm.items()) if k != "total_s")
        print(f"{name:30s} {dt:8.3f} s  ({parts})", flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=17)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--no-eager", action="store_true")
    p.add_argument("--kernels-only", action="store_true")
    a = p.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    kernels()
    if not a.kernels_only:
        whole_call(a.frames, a.steps, eager=not a.no_eager)
