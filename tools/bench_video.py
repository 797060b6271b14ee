#!/usr/bin/env python
"""Frame-sequence editing on MI355X:
  1. afldm_attention_bank against afldm_attention_interp at every FFHQ attention level, batch 16, bf16, the same two stored
     samples: all blend weights non-zero (the same arithmetic), and half of the rows with alpha 0 (those skip source 1).  The
     launches are timed in alternation, several rounds each (HIP-graph timing: 20 calls per graph, us per call), so that the
     run-to-run spread of ONE launch is on the page next to the difference between two;
  2. a whole 16-frame, 50-step LDMVideoPipeline call (FFHQ-size UNet + AF-VAE, seeded random weights, bf16): the graph path
     (first call = capture, then replays) against use_graph=False (the reference's loop statement by statement);
  3. --bank-bytes (needs no GPU): what a stored keyframe costs, from the FFHQ UNet's config."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

LEVELS = [("32^2", 1024, 192, 8), ("16^2", 256, 384, 16), ("8^2", 64, 384, 16), ("4^2", 16, 768, 32), ("2^2", 4, 768, 32)]


def kernels(B=16, dtype=torch.bfloat16, rounds=5):
    from afldm_amd import ops
    from bench_kernels import timeit_graph
    print(f"== kernel: batch {B}, {dtype}, a bank of 2 stored samples, us per call: median [min .. max] of {rounds} alternated rounds",
          flush=True)
    for name, T, C, heads in LEVELS:
        g = torch.Generator().manual_seed(T)
        q = torch.randn(B, T, C, generator=g).to(device="cuda", dtype=dtype)
        bank = torch.randn(2, T, 2 * C, generator=g).to(device="cuda", dtype=dtype)[:, :, C:]
        vt = torch.randn(2, C, T, generator=g).to(device="cuda", dtype=dtype)
        src = torch.tensor([[0, 1]] * B, dtype=torch.int32, device="cuda")
        full = torch.linspace(0.1, 0.9, B, device="cuda")
        half = full.clone()
        half[::2] = 0.0
        out = torch.empty(B, T, C, device="cuda", dtype=dtype)
        runs = [("interp", lambda: ops.attention_interp(q, bank[0:1], vt[0:1], bank[1:2], vt[1:2], full, heads, out=out)),
                ("bank", lambda: ops.attention_bank(q, bank, vt, src, full, heads, out=out)),
                ("bank, half the rows alpha 0", lambda: ops.attention_bank(q, bank, vt, src, half, heads, out=out)),
                ("1 x attention", lambda: ops.attention(q, bank[0:1], vt[0:1], heads, out=out))]
        assert torch.equal(runs[0][1](), ops.attention_bank(q, bank, vt, src, full, heads))       # (the same bits, at the sizes timed)
        times = {n: [] for n, _ in runs}
        for _ in range(rounds):
            for n, fn in runs:
                times[n].append(timeit_graph(fn))
        cells = " | ".join(f"{n} {statistics.median(t):7.1f} [{min(t):6.1f} .. {max(t):6.1f}]" for n, t in times.items())
        print(f"{name:5s} T={T:4d} C={C:3d} heads={heads:2d}: {cells}", flush=True)


def bank_bytes(steps=50):
    """Per keyframe and step: the K [T, C] + V^T [C, T] a STORE pass caches at every attention site and the map [T, C] it keeps as
    the reference does, summed over the sites the FFHQ config creates (level by level: T = side^2 tokens of C channels)."""
    from afldm_amd.configs import FFHQ_UNET_CONFIG as cfg
    side, ch, lpb = cfg["sample_size"], cfg["block_out_channels"], cfg["layers_per_block"]
    sites = []                                                    # (tokens, channels)
    for i, kind in enumerate(cfg["down_block_types"]):
        sites += [((side >> i) ** 2, ch[i])] * (lpb if kind.startswith("Attn") else 0)
    sites += [((side >> (len(ch) - 1)) ** 2, ch[-1])] * int(cfg.get("add_attention", True))
    for i, kind in enumerate(cfg["up_block_types"]):
        j = len(ch) - 1 - i
        sites += [((side >> j) ** 2, ch[j])] * ((lpb + 1) if kind.startswith("Attn") else 0)
    kv = sum(2 * t * c for t, c in sites)
    maps = sum(t * c for t, c in sites)
    print(f"== bank: {len(sites)} attention sites; per keyframe and step K + V^T {kv} elements, maps {maps} elements")
    for name, size in (("bf16", 2), ("fp32", 4)):
        per_step = (kv + maps) * size
        per_key = per_step * steps * 2                            # two samplers: the inversion's and the forward schedule's
        print(f"{name}: K + V^T {kv * size / 1e6:.2f} MB + maps {maps * size / 1e6:.2f} MB = {per_step / 1e6:.2f} MB per keyframe and step; "
              f"{steps} steps x 2 samplers = {per_key / 1e9:.3f} GB per keyframe; {int(256e9 // per_key)} keyframes in 256 GB", flush=True)


def whole_call(frames=16, steps=50, keyframes=(0, 8), dtype=torch.bfloat16, eager=True):
    import video_editing_ffhq as script
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    args = script.parse_args(["--random-init"])
    pipe = script.build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    size = pipe.unet.config.sample_size * pipe._vae_ratio()
    clip = script.synthetic_frames(1234, frames, size)
    print(f"== whole call: {frames} frames, {steps} DDIM steps (inversion + STORE + LOAD), keyframes {keyframes}, frame_batch 16, "
          f"FFHQ-size UNet + AF-VAE, {dtype}, output_type='pt'", flush=True)
    runs = [("graph, first call (captures)", True), ("graph, replay", True), ("graph, replay", True)]
    if eager:
        runs.append(("use_graph=False", False))
    for name, graph in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(clip, num_inference_steps=steps, keyframes=keyframes, output_type="pt", use_graph=graph)
        torch.cuda.synchronize()
        print(f"{name:30s} {time.perf_counter() - t0:8.3f} s", flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--keyframes", type=str, default="0,8")
    p.add_argument("--no-eager", action="store_true")
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--bank-bytes", action="store_true")
    a = p.parse_args()
    if a.bank_bytes:
        bank_bytes(a.steps)
        sys.exit(0)
    print("device:", torch.cuda.get_device_name(0), flush=True)
    kernels()
    if not a.kernels_only:
        whole_call(a.frames, a.steps, tuple(int(k) for k in a.keyframes.split(",")), eager=not a.no_eager)
