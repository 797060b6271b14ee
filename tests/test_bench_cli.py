"""bench.py's command line: --steps is the number of timed steps, and --dump-outputs writes what the timed path
computed in its last step (capped in size by a seeded row sample)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("steps,regions,spg", [(50, 5, 5), (20, 5, 5), (12, 5, 5), (7, 5, 5), (3, 5, 5), (1, 5, 5),
                                               (13, 5, 1), (13, 1, 5), (100, 3, 5)])
def test_region_steps_sum_to_steps(steps, regions, spg):
    import bench
    sizes = bench.region_steps(steps, regions, spg)
    assert sum(sizes) == steps and 1 <= len(sizes) <= regions
    assert max(sizes) - min(sizes) <= 1
    assert len(sizes) == 1 or min(sizes) >= spg


def test_dump_outputs_writes_float32_and_caps_with_a_fixed_sample(tmp_path):
    import bench
    small = torch.randn(8, 4, 32, 32, generator=torch.Generator().manual_seed(1))
    rec = bench.dump_outputs(str(tmp_path / "a"), {"latents": small})
    got = np.load(tmp_path / "a" / "latents.npy")
    assert got.dtype == np.float32 and rec["latents"]["sampled_rows"] is None
    assert np.array_equal(got, small.numpy())
    # over the cap: a seeded sample of rows, in order, identical from call to call
    big = torch.randn(64, 4, 32, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    cap = 10 * 4 * 32 * 32 * 4
    r1 = bench.dump_outputs(str(tmp_path / "b"), {"latents": big}, max_bytes=cap)
    r2 = bench.dump_outputs(str(tmp_path / "c"), {"latents": big}, max_bytes=cap)
    b1, b2 = np.load(tmp_path / "b" / "latents.npy"), np.load(tmp_path / "c" / "latents.npy")
    assert b1.dtype == np.float32 and b1.nbytes <= cap and b1.shape == (10, 4, 32, 32)
    assert np.array_equal(b1, b2) and r1 == r2 and r1["latents"]["sampled_rows"]
    rows = [int(np.flatnonzero((big.float().numpy() == b).all(axis=(1, 2, 3)))[0]) for b in b1]
    assert rows == sorted(rows) and len(set(rows)) == 10


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_latents_of_the_last_timed_step(tmp_path):
    """bench.py --steps 12 times exactly 12 steps and dumps the latents after the 12th: the same as a fresh engine run of
    12 steps from the bench's seeded weights and noise."""
    out = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "12", "--warmup", "2", "--no-cpu-baseline", "--no-extras",
           "--no-roofline", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads(lines[0])
    assert d["steps"] == 12 and sum(d["config"]["region_steps"]) == 12 and d["config"]["latents_finite"]
    assert d["dump_outputs"]["arrays"]["latents"]["shape"] == [64, 4, 32, 32]
    got = torch.from_numpy(np.load(out / "latents.npy"))
    assert got.dtype == torch.float32 and got.shape == (64, 4, 32, 32) and torch.isfinite(got).all()

    import bench
    from afldm_amd import parallel
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    torch.cuda.set_device(0)
    eng = DenoiseEngine(bench.build_unet(torch.bfloat16, torch.device("cuda", 0)), ffhq_ddim_scheduler(), 64, 50)
    noise = parallel.global_noise(64, (4, 32, 32), 1234)
    eng.reset(noise)
    eng.step(11)
    prev = eng.lat.cpu()
    eng.step(1)
    ref = eng.lat.cpu()
    rel = lambda a, b: float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    print(f"[bench dump] vs engine step 12: {rel(got, ref):.3e}; step 11 vs 12: {rel(prev, ref):.3e}")
    assert rel(got, ref) <= 1e-3 and rel(prev, ref) > 10 * max(rel(got, ref), 1e-6)


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_line_only():
    """A plain run (no --full) sets up, warms up, times its steps and prints the result line; the records that take runs
    of their own (box fingerprint, roofline, side configurations and workloads, CPU baseline) come only with --full."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads(lines[0])
    assert d["unit"] == "denoise-steps/s" and d["higher_is_better"] is True and d["dtype"] == "bf16" and d["n_gpus"] == 1
    assert d["steps"] == 5 and sum(d["config"]["region_steps"]) == 5 and d["config"]["latents_finite"]
    assert d["value"] > 0 and abs(d["value"] - 64e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    full_only = {"rccl", "box", "roofline", "kernel_families", "step_dense", "other_configs", "concurrent_jobs", "vae_c4",
                 "harness_c1", "i2sb_c5", "cpu_baseline"}
    assert not full_only & set(d), sorted(full_only & set(d))
