#!/usr/bin/env python
"""Timings of parallel-in-time sampling on MI355X: FFHQ size, bf16, ONE image.  One JSON line per measurement.

  python tools/bench_picard.py iteration [W ...]   (a) PicardEngine at a window of W (default 4 8 16 32) at tolerance 0 - 50
                                      #     iterations finish a 50-step schedule - against the plain DenoiseEngine at batch W: ms
                                      #     per iteration against ms per step (HIP events around 50 replayed ones), in alternated
                                      #     pairs in one process.  The difference is what the sweep, the stride decision with its
                                      #     gather of W time-embedding rows, and the slide cost
  python tools/bench_picard.py sample [W]   (b) one 50-step sample: pipe(batch_size=1) against sample_parallel_latents at a window
                                      #     of W (default 8) at tolerance 0 (the sequential sampler's bits; 50 iterations unless
                                      #     estimates repeat bit for bit) and at the default tolerance; HIP events around the
                                      #     whole call and the host clock, alternated rounds.  The weights are RANDOM: the
                                      #     iteration counts say nothing about a trained model
The plain engine's path is not touched by the parallel sampler, so it stands for the parent commit's engine on the same box."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_pag import median  # noqa: E402
from bench_slots import _pipe, build_unet  # noqa: E402

STEPS = 50


def iteration(windows=(4, 8, 16, 32), rounds=4):
    from afldm_amd.engine import DenoiseEngine, PicardEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = build_unet()
    sched = ffhq_ddim_scheduler().schedule(STEPS)
    for W in windows:
        plain = DenoiseEngine(unet, sched, W, STEPS)
        picard = PicardEngine(unet, sched, 1, STEPS, window=W, tolerance=0.0)
        x = torch.randn(W, 4, 32, 32, generator=torch.Generator().manual_seed(W))

        def timed(eng, start):
            start()
            eng.step(5)                                # (captures on the first call)
            start()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.step(STEPS)
            e1.record()
            torch.cuda.synchronize()
            eng.check_errors()
            return e0.elapsed_time(e1) / STEPS

        res = {"plain": [], "picard": []}
        for _ in range(rounds):
            res["plain"].append(timed(plain, lambda: plain.reset(x)))
            res["picard"].append(timed(picard, lambda: picard.reset(x[:1])))
        base, done = picard._poll()
        out = {k: dict(median=round(median(v), 4), all=[round(t, 4) for t in v]) for k, v in res.items()}
        diffs = [round(b - a, 4) for a, b in zip(res["plain"], res["picard"])]
        print(json.dumps(dict(what="iteration", window=W, images=1, steps=STEPS, rounds=rounds, unit="ms per iteration / per step",
                              finished=base == [STEPS], iterations=done, pair_differences=diffs,
                              pair_difference_median=round(median(diffs), 4), **out)), flush=True)
        del plain, picard


def sample(W=8, rounds=4):
    unet = build_unet()
    pipe = _pipe(unet)
    x = torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(1))
    counts = {}

    def parallel(name, **kw):
        own = _pipe(unet)                              # a pipeline keeps ONE engine per sampler: one pipeline per tolerance

        def run():
            _, stats = own.sample_parallel_latents(latents=x, num_inference_steps=STEPS, window=W, **kw)
            counts[name] = stats["iterations"]
        return run
    cases = {"sequential": lambda: pipe(latents=x, num_inference_steps=STEPS, output_type="latent"),
             "parallel_tolerance_0": parallel("parallel_tolerance_0", tolerance=0.0),
             "parallel_default_tolerance": parallel("parallel_default_tolerance")}
    for fn in cases.values():
        fn()                                           # captures, packs
        torch.cuda.synchronize()
    ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            ev[name].append(e0.elapsed_time(e1))
    for name in cases:
        print(json.dumps(dict(what="sample", case=name, window=W, steps=STEPS, images=1, rounds=rounds, unit="ms per sample",
                              iterations=counts.get(name, STEPS), random_weights=True, events_ms=round(median(ev[name]), 3),
                              events_all=[round(t, 3) for t in ev[name]], wall_ms=round(median(wall[name]), 3),
                              wall_all=[round(t, 3) for t in wall[name]])), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "iteration"
    rest = [int(v) for v in sys.argv[2:]]
    if what == "iteration":
        iteration(tuple(rest) or (4, 8, 16, 32))
    else:
        sample(*rest[:1])
