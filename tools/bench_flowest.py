#!/usr/bin/env python
"""The built-in flow estimator on MI355X, reported, not gated:
  1. one bidirectional PyramidLKFlow estimate at the defaults on two 256^2 x 3-channel images (6 levels, 3 iterations,
     radius 3): eager wall time (launch + Python overhead included, which is what a pipeline call pays) and as a replayed HIP
     graph (20 estimates per graph), plus the graph time of the single kernels at level 0;
  2. a whole 17-frame, 50-step LDMInterpolationPipeline call (FFHQ-size UNet + AF-VAE, seeded random weights, bf16) with
     warp_method=0: flows estimated by the pipeline (flow_model=PyramidLKFlow()) against the same call with the same flows
     precomputed and passed as flows=."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402


def wall(fn, iters=20):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def estimate(S=256):
    import image_interpolation_ffhq as script
    from afldm_amd import ops
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow
    from bench_kernels import timeit_graph
    images = [x.cuda() for x in script.synthetic_images(1234, S)]
    flow = PyramidLKFlow()
    fwd, bwd = flow(*images)
    launches = 4 + (6 - 1) * 2 + 6 * 3 * 2 + 1
    print(f"== one bidirectional estimate, {S}^2 x 3 channels, defaults (6 levels x 3 iterations, radius 3; {launches} launches); "
          f"|fwd| median {float(fwd.norm(dim=1).median()):.2f} px", flush=True)
    tg, tw = timeit_graph(lambda: flow(*images)), wall(lambda: flow(*images))
    print(f"HIP graph: {tg:8.1f} us | eager: {tw:8.1f} us", flush=True)
    I = torch.cat([images[0], images[1]]).contiguous()
    J = torch.cat([images[1], images[0]]).contiguous()
    u, out = torch.cat([fwd, bwd]).contiguous(), torch.empty(2, 2, S, S, device="cuda")
    half = torch.empty(2, 3, S // 2, S // 2, device="cuda")
    uh = ops.flowest_pyr_down(u)
    for name, fn in (("lk_step, 16 x 16 tiles (the call's choice)", lambda: ops.flowest_lk_step(I, J, u, out=out)),
                     ("lk_step, 32 x 32 tiles", lambda: ops.flowest_lk_step(I, J, u, out=out, tile=32)),
                     ("smooth", lambda: ops.flowest_smooth(u, out=out)),
                     ("up2 (128^2 -> 256^2)", lambda: ops.flowest_up2(uh, out=out)),
                     ("pyr_down (256^2 -> 128^2, 6 planes)", lambda: ops.flowest_pyr_down(I, out=half))):
        print(f"  level 0, B = 2: {name:44s} {timeit_graph(fn):7.1f} us", flush=True)


def whole_call(frames=17, steps=50, dtype=torch.bfloat16):
    import image_interpolation_ffhq as script
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow, predict_flow
    args = script.parse_args(["--random-init"])
    pipe = script.build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    images = script.synthetic_images(1234)
    model = PyramidLKFlow()
    fwd_flow, _, bwd_flow, _ = predict_flow(model, *(x.cuda() for x in images))
    print(f"== whole call: {frames} frames, {steps} DDIM steps, FFHQ-size UNet + AF-VAE, {dtype}, output_type='pt', graph path, "
          "warp_method=0", flush=True)
    for name, fm, flows in (("flows=precomputed, first call (captures)", None, (fwd_flow, bwd_flow)),
                            ("flows=precomputed, replay", None, (fwd_flow, bwd_flow)),
                            ("flow_model=PyramidLKFlow(), replay", model, None),
                            ("flows=precomputed, replay", None, (fwd_flow, bwd_flow)),
                            ("flow_model=PyramidLKFlow(), replay", model, None)):
        tm = {}
        pipe.flow_model = fm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(*images, num_frames=frames, num_inference_steps=steps, output_type="pt", timings=tm, warp_method=0, flows=flows,
             generator=torch.Generator().manual_seed(0))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        parts = ", ".join(f"{k} {v:.4f}" for k, v in sorted(tm.items()) if k != "total_s")
        print(f"{name:42s} {dt:8.3f} s  ({parts})", flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=17)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--estimate-only", action="store_true")
    a = p.parse_args()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    estimate()
    if not a.estimate_only:
        whole_call(a.frames, a.steps)
