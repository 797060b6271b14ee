#!/usr/bin/env python
"""Timings of the seeded stochastic samplers on MI355X: FFHQ size, bf16, batch 64, 50 steps.  One JSON
line per measurement, medians of 3 after a warm-up run.

  python tools/bench_counter_noise.py sampler   # wall time of one 50-step run at batch 64 (host clock, start latents given, until
                                                # the latents are on the device and the stream is idle): sample_seeded at eta = 1
                                                # (SeededEngine: the noise made in the update's registers) against pipe(eta = 1)
                                                # with a CPU generator and with a device generator (the noise buffer filled
                                                # before the replays) and against the eta = 0 engine; alternated rounds
  python tools/bench_counter_noise.py mixed [N] # N = 256 requests cycling through DDIM 50, seeded 50 (eta = 1) and DPM 20 on one
                                                # server of 64 slots built with kinds=("ddim", "dpm", "seeded"), against the same
                                                # requests in plain batches of 64 grouped by schedule (a partial batch is padded)
The generator-driven path is not touched by the seeded samplers, so it stands for the parent commit's on the same machine."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_pag import median  # noqa: E402
from bench_slots import _dpm, _pipe, build_unet  # noqa: E402

B, STEPS, REQUESTS, ROUNDS = 64, 50, 256, 3


def sampler():
    pipe = _pipe(build_unet())
    x = torch.randn(B, 4, 32, 32)
    seeds = list(range(1000, 1000 + B))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def device_generator():
        return torch.Generator(device="cuda").manual_seed(5)
    cases = {
        "seeded_eta1": lambda: pipe.sample_seeded(seeds, eta=1.0, num_inference_steps=STEPS, latents=x, output_type="latent"),
        "generator_cpu_eta1": lambda: pipe(eta=1.0, num_inference_steps=STEPS, latents=x, output_type="latent",
                                           generator=torch.Generator().manual_seed(5)),
        "generator_device_eta1": lambda: pipe(eta=1.0, num_inference_steps=STEPS, latents=x, output_type="latent",
                                              generator=device_generator()),
        "ddim_eta0": lambda: pipe(eta=0.0, num_inference_steps=STEPS, latents=x, output_type="latent"),
    }
    res = {}
    for _ in range(ROUNDS):
        for name, fn in cases.items():
            fn()                                           # warm-up: pipe keeps ONE engine per cache slot, so a case that follows
                                                           # another kind rebuilds and re-captures here, outside the timing
            res.setdefault(name, []).append(timed(fn))
    for name, v in res.items():
        print(json.dumps(dict(what="sampler", case=name, batch=B, steps=STEPS, dtype="bf16", rounds=ROUNDS,
                              wall_s=round(median(v), 4), ms_per_step=round(1e3 * median(v) / STEPS, 4),
                              all=[round(t, 4) for t in v])), flush=True)


def mixed(REQUESTS=REQUESTS):
    from afldm_amd.engine import DenoiseEngine, SeededEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.serving import SamplingServer
    unet = build_unet()
    mix = (("ddim", 50), ("seeded", 50), ("dpm", 20))
    reqs = [mix[i % len(mix)] for i in range(REQUESTS)]
    starts = torch.randn(REQUESTS, 4, 32, 32)
    useful = sum(n for _, n in reqs)
    full = {("ddim", 50): DenoiseEngine(unet, ffhq_ddim_scheduler().schedule(50), B, 50),
            ("seeded", 50): SeededEngine(unet, ffhq_ddim_scheduler().seeded_schedule(50, 1.0), B, 50),
            ("dpm", 20): DenoiseEngine(unet, _dpm().schedule(20), B, 20)}

    def grouped():
        torch.cuda.synchronize()
        t0, evals, out = time.perf_counter(), 0, []
        for key in mix:
            idx = [j for j, r in enumerate(reqs) if r == key]
            for i in range(0, len(idx), B):
                part = idx[i:i + B]
                x = torch.zeros(B, 4, 32, 32)
                x[:len(part)] = starts[part]
                kw = {"known": [1000 + j for j in part] + [0] * (B - len(part))} if key[0] == "seeded" else {}
                out.append(full[key].run(x, **kw)[:len(part)].cpu())
                evals += key[1] * B
        return time.perf_counter() - t0, evals

    server = SamplingServer(_pipe(unet), B, 5, 1, kinds=("ddim", "dpm", "seeded"))

    def served():
        torch.cuda.synchronize()
        e0, t0 = server.evaluations, time.perf_counter()
        tickets = [server.submit(n, latents=starts[i:i + 1], solver=None if s == "seeded" else s,
                                 eta=1.0 if s == "seeded" else 0.0, seed=1000 + i) for i, (s, n) in enumerate(reqs)]
        server.run()
        for t in tickets:
            t.result()
        return time.perf_counter() - t0, server.evaluations - e0

    cases = {"plain_grouped_by_schedule": grouped, "server_1x64": served}
    for fn in cases.values():
        fn()
    res = {}
    for _ in range(ROUNDS):
        for name, fn in cases.items():
            res.setdefault(name, []).append(fn())
    for name, v in res.items():
        print(json.dumps(dict(what="mixed_seeded", case=name, requests=REQUESTS, mix=mix, useful_evaluations=useful,
                              slot_evaluations=v[0][1], useful_share=round(useful / v[0][1], 4),
                              wall_s=round(median([t for t, _ in v]), 4), all=[round(t, 4) for t, _ in v],
                              useful_evaluations_per_s=round(useful / median([t for t, _ in v]), 1), rounds=ROUNDS)), flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    if len(argv) > 1:
        mixed(REQUESTS=int(argv[1]))
    else:
        {"sampler": sampler, "mixed": mixed}[argv[0] if argv else "sampler"]()
