#!/usr/bin/env python
"""Timings of self-attention guidance on MI355X, HIP-event timed, every comparison in alternated rounds in
one process.  One JSON line per measurement.

  python tools/bench_sag.py kernels   # afldm_attn_key_mass beside afldm_attention at the five FFHQ sites, batch 32 and 64; the degrade launch
  python tools/bench_sag.py step      # SAGEngine at batch 32 against the plain engine at batch 32: ms per step, and twice the plain step
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from afldm_amd import ops  # noqa: E402
from bench_pag import median, timeit_graph  # noqa: E402

LEVELS = [(1024, 192), (256, 384), (64, 384), (16, 768), (4, 768)]      # (tokens, channels) of the FFHQ UNet's attention blocks
HEAD_DIM = 24


def kernels(rounds=5):
    dt = torch.bfloat16
    for B in (32, 64):
        for T, C in LEVELS:
            heads = C // HEAD_DIM
            qk = torch.randn(B, T, 2 * C, device="cuda").to(dt)
            q, k = qk[:, :, :C], qk[:, :, C:]                  # the two halves of the buffer ops.linear_split writes
            vt = torch.randn(B, C, T, device="cuda").to(dt)
            o = torch.empty(B, T, C, device="cuda", dtype=dt)
            mass = torch.empty(B, T, device="cuda")
            a, b = [], []
            for _ in range(rounds):
                a.append(timeit_graph(lambda: ops.attn_key_mass(q, k, heads, out=mass)))
                b.append(timeit_graph(lambda: ops.attention(q, k, vt, heads, out=o)))
            print(json.dumps(dict(what="key_mass", B=B, T=T, C=C, heads=heads, key_mass_us=round(median(a), 2),
                                  attention_us=round(median(b), 2), rounds=rounds)), flush=True)
    # the degradation, FFHQ latents, the 8 x 8 site's map, beside the layout change it replaces in front of the second evaluation
    for B in (32, 64):
        x = torch.randn(B, 4, 32, 32, device="cuda")
        e = torch.randn(B, 32, 32, 4, device="cuda").to(dt)
        mass = 1.0 + 0.04 * torch.randn(B, 64, device="cuda")
        out = torch.empty_like(e)
        coef = torch.tensor([1 / 0.6, -0.8 / 0.6] + [0.0] * 10, dtype=torch.float32, device="cuda")
        idx = torch.zeros(1, dtype=torch.int32, device="cuda")
        taps = ops.gaussian_taps()
        res = {"sag_degrade_reflect": [], "sag_degrade_circular": [], "to_nhwc": []}
        for _ in range(rounds):
            res["sag_degrade_reflect"].append(timeit_graph(lambda: ops.sag_degrade(x, e, mass, taps, "reflect", coef, idx, out=out)))
            res["sag_degrade_circular"].append(timeit_graph(lambda: ops.sag_degrade(x, e, mass, taps, "circular", coef, idx, out=out)))
            res["to_nhwc"].append(timeit_graph(lambda: ops.to_nhwc(x, dt, out=out)))
        print(json.dumps(dict(what="degrade", B=B, **{k: round(median(v), 2) for k, v in res.items()}, unit="us", rounds=rounds)), flush=True)


def step(rounds=4, steps=50, B=32):
    from afldm_amd.af_modules.af_api import make_af_unet
    from afldm_amd.configs import FFHQ_UNET_CONFIG
    from afldm_amd.engine import DenoiseEngine, SAGEngine
    from afldm_amd.models.unet_2d import UNet2DModel
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    torch.manual_seed(0)
    unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG)
    with torch.no_grad():
        unet.conv_out.weight.mul_(0.1)
        unet.conv_out.bias.mul_(0.1)
    make_af_unet(unet)
    unet = unet.to("cuda").to(torch.bfloat16)
    sched = ffhq_ddim_scheduler()
    engines = {"plain_batch32": DenoiseEngine(unet, sched.schedule(steps), B, steps)}
    for name, site in {"sag_batch32_8x8_up": "up_blocks.2.attentions.0", "sag_batch32_32x32_up": "up_blocks.4.attentions.0",
                       "sag_batch32_mid_block": "mid_block.attentions.0"}.items():
        engines[name] = SAGEngine(unet, sched.sag_schedule(steps, 0.0, 0.75, 0.0), B, steps, site=site, taps=ops.gaussian_taps(),
                                  boundary="reflect")

    def run(eng):
        eng.reset(torch.randn(eng.B, 4, 32, 32))
        eng.step(5)                                    # (captures on the first call)
        eng.reset(torch.randn(eng.B, 4, 32, 32))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step(steps)
        e1.record()
        torch.cuda.synchronize()
        eng.check_errors()
        return e0.elapsed_time(e1) / steps

    res = {}
    for _ in range(rounds):
        for name, eng in engines.items():
            res.setdefault(name, []).append(run(eng))
    out = {k: dict(median=round(median(v), 4), all=[round(t, 4) for t in v]) for k, v in res.items()}
    print(json.dumps(dict(what="step", steps=steps, rounds=rounds, unit="ms/step",
                          two_plain_steps=round(2 * out["plain_batch32"]["median"], 4), **out)), flush=True)


if __name__ == "__main__":
    {"kernels": kernels, "step": step}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
