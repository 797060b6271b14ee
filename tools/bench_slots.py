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
  python tools/bench_slots.py step --solver dpm    (a) with DPM-Solver++ in slots: a SlotEngine built with kinds=("ddim", "dpm"), all
                                      #     64 slots in phase on one 20-step "dpm" schedule, against the plain DenoiseEngine on
                                      #     the same schedule; and a 50-step "ddim" schedule on that engine against a default
                                      #     SlotEngine - what the 8-wide rows, the kind lookup and the history planes cost
  python tools/bench_slots.py mixed [N] --solver dpm  (b) N = 256 requests cycling through DDIM 50, DPM 20 and DPM 25 on one server of
                                      #     64 slots, against the same requests in plain batches: in arrival order (every chunk of
                                      #     64 runs one plain batch per schedule it holds) and grouped by schedule
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


def _dpm():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG)


def _pairs(what, a, b, fill_a, fill_b, steps, rounds, names):
    """ms per replayed step of engines a and b in alternated pairs; fill_x() puts x at the start of the schedule."""
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
    res = {names[0]: [], names[1]: []}
    for _ in range(rounds):
        res[names[0]].append(timed(a, fill_a))
        res[names[1]].append(timed(b, fill_b))
    same = torch.equal(a.lat, b.lat)
    out = {k: dict(median=round(median(v), 4), all=[round(t, 4) for t in v]) for k, v in res.items()}
    print(json.dumps(dict(what=what, batch=B, steps=steps, rounds=rounds, unit="ms/step", bit_identical_latents=same,
                          pair_differences=[round(y - x, 4) for x, y in zip(res[names[0]], res[names[1]])], **out)), flush=True)


def step_dpm(rounds=4):
    from afldm_amd.engine import DenoiseEngine, SlotEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = build_unet()
    x = torch.randn(B, 4, 32, 32)
    dpm, ddim = _dpm().schedule(20), ffhq_ddim_scheduler().schedule(50)
    plain, kinds, default = DenoiseEngine(unet, dpm, B, 20), SlotEngine(unet, B, kinds=("ddim", "dpm")), SlotEngine(unet, B)
    dpm_span, ddim_span, default_span = kinds.add_schedule(dpm), kinds.add_schedule(ddim), default.add_schedule(ddim)

    def fill(eng, span):
        return lambda: eng.exchange({}, {b: (x[b], *span) for b in range(B)})
    _pairs("step_dpm", plain, kinds, lambda: plain.reset(x), fill(kinds, dpm_span), 20, rounds, ("plain_dpm", "slots_dpm"))
    _pairs("step_ddim_on_kinds_engine", default, kinds, fill(default, default_span), fill(kinds, ddim_span), 50, rounds,
           ("slots_default", "slots_kinds"))


def mixed_dpm(rounds=3, REQUESTS=REQUESTS):
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.serving import SamplingServer
    unet = build_unet()
    mix = (("ddim", 50), ("dpm", 20), ("dpm", 25))
    reqs = [mix[i % len(mix)] for i in range(REQUESTS)]
    starts = torch.randn(REQUESTS, 4, 32, 32)
    useful = sum(n for _, n in reqs)
    sched = {(s, n): (ffhq_ddim_scheduler() if s == "ddim" else _dpm()).schedule(n) for s, n in mix}
    per = -(-B // len(mix))                            # a chunk of 64 in arrival order holds at most this many of one schedule
    small = {k: DenoiseEngine(unet, v, per, k[1]) for k, v in sched.items()}
    full = {k: DenoiseEngine(unet, v, B, k[1]) for k, v in sched.items()}

    def batches(engines, width, groups):
        torch.cuda.synchronize()
        t0, evals, out = time.perf_counter(), 0, []
        for key, idx in groups:
            x = torch.zeros(width, 4, 32, 32)
            x[:len(idx)] = starts[idx]
            out.append(engines[key].run(x)[:len(idx)].cpu())
            evals += key[1] * width
        return time.perf_counter() - t0, evals

    def arrival():
        groups = []
        for i in range(0, REQUESTS, B):
            for key in mix:
                idx = [j for j in range(i, min(i + B, REQUESTS)) if reqs[j] == key]
                if idx:
                    groups.append((key, idx))
        return batches(small, per, groups)

    def grouped():
        groups = []
        for key in mix:
            idx = [j for j, r in enumerate(reqs) if r == key]
            groups += [(key, idx[i:i + B]) for i in range(0, len(idx), B)]
        return batches(full, B, groups)

    server = SamplingServer(_pipe(unet), B, 5, 1, kinds=("ddim", "dpm"))

    def served():
        torch.cuda.synchronize()
        e0, t0 = server.evaluations, time.perf_counter()
        tickets = [server.submit(n, latents=starts[i:i + 1], solver=s) for i, (s, n) in enumerate(reqs)]
        server.run()
        for t in tickets:
            t.result()
        return time.perf_counter() - t0, server.evaluations - e0

    cases = {f"plain_arrival_order_batch_{per}_per_schedule": arrival, "plain_grouped_by_schedule": grouped, "server_1x64": served}
    for fn in cases.values():
        fn()
    res = {}
    for _ in range(rounds):
        for name, fn in cases.items():
            res.setdefault(name, []).append(fn())
    for name, v in res.items():
        print(json.dumps(dict(what="mixed_dpm", case=name, requests=REQUESTS, mix=mix, useful_evaluations=useful,
                              slot_evaluations=v[0][1], useful_share=round(useful / v[0][1], 4),
                              wall_s=round(median([t for t, _ in v]), 4), all=[round(t, 4) for t, _ in v],
                              useful_evaluations_per_s=round(useful / median([t for t, _ in v]), 1), rounds=rounds)), flush=True)


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
    argv, solver = sys.argv[1:], "ddim"
    if "--solver" in argv:
        i = argv.index("--solver")
        solver = argv[i + 1]
        del argv[i:i + 2]
        if solver not in ("ddim", "dpm"):
            sys.exit("--solver ddim | dpm")
    modes = {"step": step, "mixed": mixed} if solver == "ddim" else {"step": step_dpm, "mixed": mixed_dpm}
    if len(argv) > 1:
        modes["mixed"](REQUESTS=int(argv[1]))
    else:
        modes[argv[0] if argv else "step"]()
