#!/usr/bin/env python
"""Timings of perturbed-attention guidance on MI355X, HIP-event timed, every comparison in alternated rounds
in one process.  One JSON line per measurement.

  python tools/bench_pag.py kernels   # the identity-block launch against gn_apply + conv2d per level, afldm_pag_step against afldm_sde_step
  python tools/bench_pag.py step      # PAGEngine at batch 32 (64 UNet rows) against the plain engine at batch 64, ms per step
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from afldm_amd import ops  # noqa: E402


def timeit_graph(fn, reps=20, iters=10):
    """us per call with `reps` calls captured into one HIP graph (an eager call's ~20 us of Python hides anything shorter)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (iters * reps) * 1e3


LEVELS = [(1024, 192), (256, 384), (64, 384), (16, 768), (4, 768)]      # (tokens, channels) of the FFHQ UNet's attention blocks
G, EPS = 32, 1e-5


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def kernels(B=32, rounds=5):
    dt = torch.bfloat16
    ops._IDENTITY_MIN_T = 4                            # the one launch at every level it has a kernel for, whatever the policy
    for T, C in LEVELS:
        x = (torch.randn(B, T, C, device="cuda") * 1.5 + 0.5).to(dt)
        gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        w = ops.pack_weight(torch.randn(C, C, device="cuda") / C ** 0.5, dt)
        bias = torch.zeros(C, device="cuda")
        stats = ops.gn_stats(x, G)
        out = torch.empty_like(x)
        hn = torch.empty_like(x)

        def fused():
            ops.attn_identity_block(x, stats, gamma, beta, G, EPS, w, bias, out=out)

        def composed():
            ops.gn_apply(x, stats, gamma, beta, G, EPS, act=0, out=hn)
            ops.conv2d(hn, w, bias, residual=x, out=out)

        assert ops.attn_identity_block_ok(x, G)
        a, b = [], []
        for _ in range(rounds):
            a.append(timeit_graph(fused))
            b.append(timeit_graph(composed))
        print(json.dumps(dict(what="identity_block", B=B, T=T, C=C, one_launch_us=round(median(a), 2),
                              gn_apply_conv2d_us=round(median(b), 2), rounds=rounds)), flush=True)
    # the guided update against the stochastic update, FFHQ latents
    x = torch.randn(B, 4, 32, 32, device="cuda")
    eps2 = torch.randn(2 * B, 32, 32, 4, device="cuda").to(dt)
    noise = torch.randn(1, B, 4, 32, 32, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    row = (1 / 0.6, -0.8 / 0.6, -float("inf"), float("inf"), 0.0, 0.7, 0.5, 0.3)
    sde = torch.tensor(row, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    res = {}
    cases = {"sde_step": lambda: ops.sde_step(x, eps2[:B], noise, sde, idx, out=out)}
    for name, (s, phi) in {"pag_step_phi0": (3.0, 0.0), "pag_step_phi07": (3.0, 0.7)}.items():
        coef = torch.tensor(row + (s, phi, 0.0, 0.0), dtype=torch.float32, device="cuda")
        cases[name] = lambda coef=coef: ops.pag_step(x, eps2, noise, coef, idx, out=out)
    for _ in range(rounds):
        for name, fn in cases.items():
            res.setdefault(name, []).append(timeit_graph(fn))
    print(json.dumps(dict(what="update", B=B, **{k: round(median(v), 2) for k, v in res.items()}, unit="us", rounds=rounds)), flush=True)


def step(rounds=4, steps=50):
    from afldm_amd.af_modules.af_api import make_af_unet
    from afldm_amd.configs import FFHQ_UNET_CONFIG
    from afldm_amd.engine import DenoiseEngine, PAGEngine
    from afldm_amd.models.unet_2d import UNet2DModel
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    torch.manual_seed(0)
    unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG)
    with torch.no_grad():
        unet.conv_out.weight.mul_(0.1)
        unet.conv_out.bias.mul_(0.1)
    make_af_unet(unet)
    unet = unet.to("cuda").to(torch.bfloat16)
    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    sched = ffhq_ddim_scheduler()
    engines = {"plain_batch64": DenoiseEngine(unet, sched.schedule(steps), 64, steps)}
    for name, layers in {"pag_batch32_mid_block": ("mid_block",), "pag_batch32_8_4_2": ("down_blocks.2", "down_blocks.3", "mid_block")}.items():
        engines[name] = PAGEngine(unet, sched.pag_schedule(steps, 0.0, 3.0, 0.0), 32, steps, sites=pipe.pag_sites(layers))

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
    print(json.dumps(dict(what="step", steps=steps, rounds=rounds, unit="ms/step",
                          **{k: dict(median=round(median(v), 4), all=[round(t, 4) for t in v]) for k, v in res.items()})), flush=True)


if __name__ == "__main__":
    {"kernels": kernels, "step": step}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
