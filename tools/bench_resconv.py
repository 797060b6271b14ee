#!/usr/bin/env python
"""The vanilla resamplers' convolutions on MI355X (csrc/resconv.hip), bf16, B = 64.

  python tools/bench_resconv.py kernels   # every s2 / up2 site + the stride-1 3x3 conv at 256^2 for comparison, 10 calls
                                          # each: run under `rocprofv3 --kernel-trace --stats` for the kernel times
  python tools/bench_resconv.py step      # ms per denoise step (graph replay) of the vanilla and the alias-free FFHQ UNet

FLOP counts for the report: s2 = 2 M Cout 9 Cin with M = B (H/2) (W/2); up2 literal = 2 (4 B H W) Cout 9 Cin (the
convolution of the x2 plane), folded = 2 (4 B H W) Cout 4 Cin (what the kernel executes)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from afldm_amd import ops  # noqa: E402

B = 64
DT = torch.bfloat16
S2 = [("unet", 192, 32), ("unet", 384, 16), ("unet", 384, 8), ("unet", 768, 4),
      ("vae", 128, 256), ("vae", 256, 128), ("vae", 512, 64)]
UP2 = [("unet", 768, 2), ("unet", 768, 4), ("unet", 384, 8), ("unet", 384, 16),
       ("vae", 512, 32), ("vae", 512, 64), ("vae", 256, 128)]


def kernels(reps=10):
    rows = []
    for kind, C, N in S2:
        x = torch.randn(B, N, N, C, device="cuda", dtype=DT)
        w = ops.pack_weight(torch.randn(C, C, 3, 3, device="cuda") * 0.02, DT)
        b = torch.zeros(C, device="cuda")
        for _ in range(reps):
            ops.conv2d_s2(x, w, b, pad=(1, 1) if kind == "unet" else (0, 1), want_stats=True)
        rows.append(dict(op="s2", site=f"{kind} {C}ch {N}->{N // 2}", flops=2.0 * B * (N // 2) ** 2 * C * 9 * C))
        del x
    for kind, C, N in UP2:
        x = torch.randn(B, N, N, C, device="cuda", dtype=DT)
        w = ops.pack_weight_up2(torch.randn(C, C, 3, 3, device="cuda") * 0.02, DT)
        b = torch.zeros(C, device="cuda")
        for _ in range(reps):
            y = ops.conv2d_up2(x, w, b, want_stats=True)
            del y
        rows.append(dict(op="up2", site=f"{kind} {C}ch {N}->{2 * N}", flops=2.0 * 4 * B * N * N * C * 9 * C,
                         flops_folded=2.0 * 4 * B * N * N * C * 4 * C))
        del x
    # the existing stride-1 3x3 family at the decoder's 256^2 plane (256 channels), for the rate comparison
    x = torch.randn(B, 256, 256, 256, device="cuda", dtype=DT)
    w = ops.pack_weight(torch.randn(256, 256, 3, 3, device="cuda") * 0.02, DT)
    b = torch.zeros(256, device="cuda")
    for _ in range(reps):
        y = ops.conv2d(x, w, b, want_stats=True)
        del y
    rows.append(dict(op="conv3x3", site="vae 256ch 256^2 stride 1", flops=2.0 * B * 256 * 256 * 256 * 9 * 256))
    torch.cuda.synchronize()
    print(json.dumps(dict(calls_per_site=reps, sites=rows)))


def step(steps=20):
    from afldm_amd.af_modules.af_api import enable_vanilla_resampling, make_af_unet
    from afldm_amd.configs import FFHQ_UNET_CONFIG
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.models.unet_2d import UNet2DModel
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    out = {}
    for name, surgery in (("vanilla", enable_vanilla_resampling), ("alias_free", make_af_unet)):
        torch.manual_seed(0)
        unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG)
        surgery(unet)
        unet = unet.to("cuda").to(DT)
        eng = DenoiseEngine(unet, ffhq_ddim_scheduler(), B, 50, use_graph=True)
        x = torch.randn(B, 4, 32, 32)
        eng.reset(x)
        eng.step(5)                       # capture + warm
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step(steps)
        e1.record()
        torch.cuda.synchronize()
        out[name] = round(e0.elapsed_time(e1) / steps, 4)
        assert torch.isfinite(eng.lat).all()
        del eng, unet
    print(json.dumps(dict(batch=B, dtype="bf16", ms_per_step=out)))


if __name__ == "__main__":
    {"kernels": kernels, "step": step}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
