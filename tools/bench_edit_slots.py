#!/usr/bin/env python
"""Timings of image-conditioned requests in slots on MI355X: FFHQ size, bf16, batch 64.  One JSON line per
measurement.

  python tools/bench_edit_slots.py step [rounds]  # ms per replayed step of an EditSlotEngine whose 64 slots all hold seeded DDIM
                                                  # requests (eta = 1, 50 steps: kind code 2 on 12-wide rows, afldm_slot_step_edit)
                                                  # against a SeededSlotEngine on the same rows (afldm_slot_step_seeded): event
                                                  # times of 45 replayed steps, alternated pairs, the pairs' differences listed
  python tools/bench_edit_slots.py mixed [N]      # N = 256 requests cycling through unconditional DDIM 50 / img2img strength 0.6 of
                                                  # 50 (30 evaluations) / RePaint n = 20, jump_length = 5, jump_n_sample = 2 (35
                                                  # evaluations), all at eta = 0, on one server of 64 slots, against the same
                                                  # requests through pipe(), pipe.img2img_latents and pipe.inpaint_latents in batches
                                                  # of 64 grouped by schedule (a partial batch is padded; RePaint's draws come from a
                                                  # device generator, the plain path's fastest)
The plain pipelines are not touched by the edit slots, so they stand for the parent commit's on the same machine."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bench_pag import median  # noqa: E402
from bench_slots import _pairs, _pipe, build_unet  # noqa: E402

B, REQUESTS, ROUNDS = 64, 256, 3
EDIT_KINDS = ("ddim", "seeded", "seeded_sdedit", "seeded_repaint")


def step(rounds=7):
    from afldm_amd.engine import EditSlotEngine, SeededSlotEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = build_unet()
    x = torch.randn(B, 4, 32, 32)
    sched = ffhq_ddim_scheduler().seeded_schedule(50, 1.0)
    seeded, edit = SeededSlotEngine(unet, B, kinds=("ddim", "seeded")), EditSlotEngine(unet, B, kinds=EDIT_KINDS)
    s_span, e_span = seeded.add_schedule(sched), edit.add_schedule(sched)

    def fill(eng, span, extra):
        return lambda: eng.exchange({}, {b: (x[b], *span, 1000 + b) + extra for b in range(B)})
    _pairs("step_seeded_rows_on_edit_engine", seeded, edit, fill(seeded, s_span, ()), fill(edit, e_span, (None, None)), 45, rounds,
           ("seeded_slot_engine", "edit_slot_engine"))


def mixed(REQUESTS=REQUESTS):
    from afldm_amd.serving import SamplingServer
    unet = build_unet()
    pipe = _pipe(unet)
    mix = (("txt", 50), ("img2img", 30), ("inpaint", 35))
    reqs = [mix[i % len(mix)] for i in range(REQUESTS)]
    g = torch.Generator().manual_seed(3)
    starts = torch.randn(REQUESTS, 4, 32, 32, generator=g)
    images = torch.randn(REQUESTS, 4, 32, 32, generator=g).cuda()          # the original / known latents of request i
    cmap = torch.rand(1, 1, 32, 32, generator=g).cuda()
    mask = (torch.rand(1, 1, 32, 32, generator=g) > 0.5).float().cuda()
    useful = sum(n for _, n in reqs)

    def grouped():
        torch.cuda.synchronize()
        t0, evals, out = time.perf_counter(), 0, []
        for key in mix:
            idx = [j for j, r in enumerate(reqs) if r == key]
            for i in range(0, len(idx), B):
                part = idx[i:i + B]
                pad = part + [part[-1]] * (B - len(part))
                if key[0] == "txt":
                    got = pipe(batch_size=B, num_inference_steps=50, latents=starts[pad], output_type="latent")
                elif key[0] == "img2img":
                    got = pipe.img2img_latents(images[pad], 0.6, cmap, 50, 0.0, generator=torch.Generator(device="cuda").manual_seed(i))
                else:
                    got = pipe.inpaint_latents(images[pad], mask, 20, 0.0, 5, 2, generator=torch.Generator(device="cuda").manual_seed(i),
                                               latents=starts[pad])
                out.append(got[:len(part)].float().cpu())
                evals += key[1] * B
        return time.perf_counter() - t0, evals

    server = SamplingServer(pipe, B, 5, 1, kinds=EDIT_KINDS)

    def served():
        torch.cuda.synchronize()
        e0, t0, tickets = server.evaluations, time.perf_counter(), []
        for i, (what, _) in enumerate(reqs):
            if what == "txt":
                tickets.append(server.submit(50, latents=starts[i:i + 1]))
            elif what == "img2img":
                tickets.append(server.submit_img2img_latents(images[i:i + 1], 0.6, cmap, 50, 0.0, seed=1000 + i))
            else:
                tickets.append(server.submit_inpaint_latents(images[i:i + 1], mask, 20, 0.0, 5, 2, seed=1000 + i))
        server.run()
        for t in tickets:
            t.result()
        return time.perf_counter() - t0, server.evaluations - e0

    cases = {"plain_grouped_by_schedule": grouped, "server_1x64": served}
    for fn in cases.values():
        fn()
    assert [len(pipe.scheduler.sdedit_schedule(50, 0.6).rows), len(pipe.scheduler.repaint_schedule(20, 0.0, 5, 2).rows)] == [30, 35]
    res = {}
    for _ in range(ROUNDS):
        for name, fn in cases.items():
            res.setdefault(name, []).append(fn())
    for name, v in res.items():
        print(json.dumps(dict(what="mixed_edit", case=name, requests=REQUESTS, mix=mix, useful_evaluations=useful,
                              slot_evaluations=v[0][1], useful_share=round(useful / v[0][1], 4),
                              wall_s=round(median([t for t, _ in v]), 4), all=[round(t, 4) for t, _ in v],
                              useful_evaluations_per_s=round(useful / median([t for t, _ in v]), 1), rounds=ROUNDS)), flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    what = argv[0] if argv else "step"
    if what == "step":
        step(*(int(a) for a in argv[1:2]))
    else:
        mixed(*(int(a) for a in argv[1:2]))
