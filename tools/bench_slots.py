#!/usr/bin/env python
"""Timings of the slot sampler on MI355X: FFHQ size, bf16, 64 slots.  One JSON line per measurement.

  python tools/bench_slots.py step    # (a) SlotEngine with all 64 slots in phase on one 50-step schedule against the plain
                                      #     DenoiseEngine at batch 64: ms per step (HIP events around 50 replayed steps), in
                                      #     alternated pairs in one process - what the per-sample embedding rows cost
  python tools/bench_slots.py mixed [N]  (b) N = 256 requests, step counts cycling through (20, 35, 50): wall time (host clock, from the
                                      #     first upload to the last result on the host) and the useful share of the slot
                                      #     evaluations, for the server with one engine and with two, and for plain
                                      #     DenoiseEngine batches of 64 in arrival order (each runs to its longest member) and
                                      #     grouped by step count (a partial batch is padded); alternated rounds
The plain engine's path is not touched by the slot sampler, so it stands for the parent commit's engine on the same box."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_pag import median  # noqa: E402

B, COUNTS, REQUESTS = 64, (20, 35, 50), 256


def build_unet():
    from afldm_amd.af_modules.af_api import make_af_unet
    from afldm_amd.configs import FFHQ_UNET_CONFIG
    from afldm_amd.models.unet_2d import UNet2DModel
    torch.manual_seed(0)
    unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG)
    with torch.no_grad():
        unet.conv_out.weight.mul_(0.1)
        unet.conv_out.bias.mul_(0.1)
    make_af_unet(unet)
    return unet.to("cuda").to(torch.bfloat16)


def _pipe(unet):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def step(rounds=4, steps=50):
    from afldm_amd.engine import DenoiseEngine, SlotEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = build_unet()
    sched = ffhq_ddim_scheduler().schedule(steps)
    plain, slots = DenoiseEngine(unet, sched, B, steps), SlotEngine(unet, B)
    span = slots.add_schedule(sched)
    x = torch.randn(B, 4, 32, 32)

    def timed(eng, start):
        start()
        eng.step(5)                                    # (captures on the first call)
        start()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step(steps)
        e1.record()
        torch.cuda.synchronize()
        eng.check_errors()
        return e0.elapsed_time(e1) / steps

    def fill():
        slots.exchange({}, {b: (x[b], *span) for b in range(B)})
    res = {"plain": [], "slots": []}
    for _ in range(rounds):
        res["plain"].append(timed(plain, lambda: plain.reset(x)))
        res["slots"].append(timed(slots, fill))
    same = torch.equal(plain.lat, slots.lat)
    out = {k: dict(median=round(median(v), 4), all=[round(t, 4) for t in v]) for k, v in res.items()}
    print(json.dumps(dict(what="step", batch=B, steps=steps, rounds=rounds, unit="ms/step", bit_identical_latents=same,
                          pair_differences=[round(b - a, 4) for a, b in zip(res["plain"], res["slots"])], **out)), flush=True)


def mixed(rounds=3, REQUESTS=REQUESTS):
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.serving import SamplingServer
    unet = build_unet()
    counts = [COUNTS[i % len(COUNTS)] for i in range(REQUESTS)]
    starts = torch.randn(REQUESTS, 4, 32, 32)
    useful = sum(counts)
    plain = {n: DenoiseEngine(unet, ffhq_ddim_scheduler().schedule(n), B, n) for n in COUNTS}

    def batches(groups):
        """Plain batches: (step count, request indices) each; -> wall seconds, slot evaluations."""
        torch.cuda.synchronize()
        t0, evals, out = time.perf_counter(), 0, []
        for n, idx in groups:
            x = torch.zeros(B, 4, 32, 32)
            x[:len(idx)] = starts[idx]
            out.append(plain[n].run(x)[:len(idx)].cpu())
            evals += n * B
        return time.perf_counter() - t0, evals

    def arrival():
        chunks = [list(range(i, min(i + B, REQUESTS))) for i in range(0, REQUESTS, B)]
        return batches([(max(counts[i] for i in c), c) for c in chunks])

    def grouped():
        groups = []
        for n in COUNTS:
            idx = [i for i, c in enumerate(counts) if c == n]
            groups += [(n, idx[i:i + B]) for i in range(0, len(idx), B)]
        return batches(groups)

    servers = {}

    def served(engines, slots):
        def run():
            key = (engines, slots)
            if key not in servers:
                servers[key] = SamplingServer(_pipe(unet), slots, 5, engines)
            s = servers[key]
            torch.cuda.synchronize()
            e0 = s.evaluations
            t0 = time.perf_counter()
            tickets = [s.submit(n, latents=starts[i:i + 1]) for i, n in enumerate(counts)]
            s.run()
            for t in tickets:
                t.result()
            return time.perf_counter() - t0, s.evaluations - e0
        return run

    cases = {"plain_arrival_order": arrival, "plain_grouped_by_steps": grouped, "server_1x64": served(1, B),
             "server_2x64": served(2, B), "server_2x32": served(2, B // 2)}
    for fn in cases.values():
        fn()                                           # captures, packs, sizes the pinned staging
    res = {}
    for _ in range(rounds):
        for name, fn in cases.items():
            res.setdefault(name, []).append(fn())
    for name, v in res.items():
        print(json.dumps(dict(what="mixed", case=name, requests=REQUESTS, counts=COUNTS, useful_evaluations=useful,
                              slot_evaluations=v[0][1], useful_share=round(useful / v[0][1], 4),
                              wall_s=round(median([t for t, _ in v]), 4), all=[round(t, 4) for t, _ in v],
                              useful_evaluations_per_s=round(useful / median([t for t, _ in v]), 1), rounds=rounds)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2:
        mixed(REQUESTS=int(sys.argv[2]))
    else:
        {"step": step, "mixed": mixed}[sys.argv[1] if len(sys.argv) > 1 else "step"]()
