#!/usr/bin/env python
"""Timings of class-conditional sampling with classifier-free guidance on MI355X, HIP-event timed, every
comparison in alternated rounds in one process, bf16, FFHQ shapes.  One JSON line per measurement.

  python tools/bench_cfg.py kernels   # afldm_cond_embed + the per-row projection GEMM at 64 and 128 rows against the afldm_select_step_row they replace
  python tools/bench_cfg.py step      # CFGEngine at batch 32 (64 UNet rows) against the plain engine at batch 64 and PAGEngine at batch 32, ms per step
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from afldm_amd import ops  # noqa: E402
from bench_pag import median, timeit_graph  # noqa: E402  (tools/ is the script's directory)


def _ffhq_unet(**kw):
    from afldm_amd.af_modules.af_api import make_af_unet
    from afldm_amd.configs import FFHQ_UNET_CONFIG
    from afldm_amd.models.unet_2d import UNet2DModel
    torch.manual_seed(0)
    unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG, **kw)
    with torch.no_grad():
        unet.conv_out.weight.mul_(0.1)
        unet.conv_out.bias.mul_(0.1)
    make_af_unet(unet)
    return unet.to("cuda").to(torch.bfloat16)


def kernels(rounds=5, n=50):
    """The head of a step: select_timestep + cond_embed + the projection GEMM, each alone and the three together, against
    select_step_row on a table of the same projection width."""
    dt = torch.bfloat16
    unet = _ffhq_unet(num_class_embeds=8)
    w, b, _, width = unet._temb_weights(dt)
    D = w.shape[-1]
    t_table = torch.arange(n, dtype=torch.float32, device="cuda")
    t_cur = torch.zeros(1, dtype=torch.float32, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    emb_table = torch.randn(n, D, device="cuda").to(dt)
    temb_table = torch.randn(n, width, device="cuda").to(dt)
    temb_row = torch.empty_like(temb_table[:1])
    for rows in (64, 128):
        cls = torch.randn(rows, D, device="cuda").to(dt)
        act, proj = torch.empty_like(cls), torch.empty(rows, width, dtype=dt, device="cuda")
        cases = {"select_step_row": lambda: ops.select_step_row(t_table, idx, t_cur, temb_table, temb_row),
                 "select_timestep": lambda: ops.select_timestep(t_table, idx, t_cur),
                 "cond_embed": lambda: ops.cond_embed(emb_table, idx, cls, out=act),
                 "projection_gemm": lambda: ops.conv2d(act, w, b, out=proj)}

        def head():
            ops.select_timestep(t_table, idx, t_cur)
            ops.cond_embed(emb_table, idx, cls, out=act)
            ops.conv2d(act, w, b, out=proj)
        cases["cfg_head"] = head
        res = {}
        for _ in range(rounds):
            for name, fn in cases.items():
                res.setdefault(name, []).append(timeit_graph(fn))
        print(json.dumps(dict(what="step_head", rows=rows, D=D, width=width, unit="us", rounds=rounds,
                              **{k: dict(median=round(median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
                                 for k, v in res.items()})), flush=True)


def step(rounds=4, steps=50):
    from afldm_amd.engine import CFGEngine, DenoiseEngine, PAGEngine
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    plain, cond = _ffhq_unet(), _ffhq_unet(num_class_embeds=8)
    sched = ffhq_ddim_scheduler()
    pipe = MyLDMPipeline(None, plain, ffhq_ddim_scheduler())
    engines = {"plain_batch64": DenoiseEngine(plain, sched.schedule(steps), 64, steps),
               "cfg_batch32": CFGEngine(cond, sched.cfg_schedule(steps, 0.0, 3.0, 0.0), 32, steps, guided=True),
               "cfg_scale1_batch64": CFGEngine(cond, sched.schedule(steps), 64, steps, guided=False),
               "pag_batch32_mid_block": PAGEngine(plain, sched.pag_schedule(steps, 0.0, 3.0, 0.0), 32, steps,
                                                  sites=pipe.pag_sites(("mid_block",)))}
    labels = torch.arange(32) % 7
    rows = {"cfg_batch32": cond.class_embed(torch.cat([labels, torch.full((32,), 7)])),
            "cfg_scale1_batch64": cond.class_embed(torch.cat([labels, labels]))}

    def run(name, eng):
        def reset():
            eng.reset(torch.randn(eng.B, 4, 32, 32))
            if name in rows:
                eng.class_rows.copy_(rows[name])
        reset()
        eng.step(5)                                    # (captures on the first call)
        reset()
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
            res.setdefault(name, []).append(run(name, eng))
    print(json.dumps(dict(what="step", steps=steps, rounds=rounds, unit="ms/step",
                          **{k: dict(median=round(median(v), 4), all=[round(t, 4) for t in v]) for k, v in res.items()})), flush=True)


if __name__ == "__main__":
    {"kernels": kernels, "step": step}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
