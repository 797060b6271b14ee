"""Parallel-in-time sampling without a GPU: the float64 restatement (tests/picard_oracle.py) against the sequential sampler
(tests/slot_oracle.py), the properties every tolerance must keep, the inputs the GPU tests use with tolerance > 0 - chosen HERE
so that no error of theirs is within a factor 2 of the threshold, which a GPU test could otherwise cross in fp32 - and the
surface: signatures, refusals, bindings."""
import inspect
import math
import os
import subprocess
import sys

import pytest
import torch

import picard_oracle as po
import slot_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the fixture of tests/test_gpu_picard_pipeline.py: the tiny UNet, 6 steps, a window of 3, two images
FIXTURE = dict(steps=6, window=3, seeds=(100, 101), tolerance=0.01)
# two images that finish after different iteration counts (2 and 3): 4 steps, a window of 3
UNEVEN = dict(steps=4, window=3, seeds=(108, 102), tolerance=0.0657)


def start(seeds):
    from afldm_amd.utils import randn_tensor
    return torch.cat([randn_tensor((1, 4, 16, 16), generator=torch.Generator().manual_seed(s)) for s in seeds])


def _schedule(n):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    return ffhq_ddim_scheduler().schedule(n)


@pytest.fixture(scope="module")
def tiny():
    from oracle import configs as oc, unet as ou
    cfg = oc.tiny_unet()
    return cfg, ou.randomize_norm_affine(ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1))      # test_gpu_unet.build("tiny", ...)


def _toy(z, r):
    """A cheap eps that depends on the state and on the row."""
    return torch.tanh(0.7 * z.double().roll(1, -1) + 0.3 * r)


def _sequential(eps_fn, x, schedule):
    z = x.double() * schedule.init_noise_sigma
    for r, row in enumerate(schedule.rows):
        z = torch.cat([so.ddim_row(z[p:p + 1], eps_fn(z[p:p + 1], r), row) for p in range(z.shape[0])])
    return z


# ------------------------------------------------------------------------------------------------ tolerance 0 and infinity
def test_tolerance_zero_is_the_sequential_sampler(tiny):
    cfg, sd = tiny
    n, x = 6, start((100,))
    sched = _schedule(n)
    want = so.sample(sd, cfg, x, sched)
    for window in (1, 3):
        got, strides, _ = po.sample(po.unet_eps(sd, cfg, sched), x, sched, window, 0.0)
        assert got.dtype == torch.float64 and torch.equal(got, want)
        assert len(strides) == n and all(s == [1] for s in strides)


@pytest.mark.parametrize("n, window", [(7, 3), (6, 3), (4, 5), (1, 2)])
def test_tolerance_infinity_takes_whole_windows(n, window):
    _, strides, _ = po.sample(_toy, start((1, 2)), _schedule(n), window, float("inf"))
    assert len(strides) == math.ceil(n / window)
    assert all(s == [window] * 2 for s in strides[:-1]) and strides[-1] == [n - window * (len(strides) - 1)] * 2


@pytest.mark.parametrize("tolerance", [0.0, 0.05, 0.5, 2.0, 20.0])
@pytest.mark.parametrize("n, window", [(7, 3), (5, 8), (6, 1)])
def test_strides_at_any_tolerance(n, window, tolerance):
    x = start((3, 4, 5))
    got, strides, errs = po.sample(_toy, x, _schedule(n), window, tolerance)
    assert 1 <= len(strides) <= n and torch.isfinite(got).all()
    base = [0] * 3
    for it in strides:
        for p, s in enumerate(it):
            assert (1 <= s <= window) if base[p] < n else s == 0
            base[p] += s
    assert base == [n] * 3
    if tolerance == 0.0:
        assert torch.equal(got, _sequential(_toy, x, _schedule(n)))


# ------------------------------------------------------------------------------------------------ eps of the row only
@pytest.mark.parametrize("n, window", [(7, 3), (7, 2), (4, 5), (1, 3), (6, 1)])
def test_row_only_eps_converges_in_one_sweep_per_window(n, window):
    table = torch.randn(n, 1, 4, 16, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
    eps_fn = lambda z, r: table[r]
    x, sched = start((6, 7)), _schedule(n)
    got, strides, _ = po.sample(eps_fn, x, sched, window, 0.0)
    assert len(strides) == po.row_only_iterations(n, window)
    if n <= window + 1 or window == 1:
        assert len(strides) == 1 + math.ceil((n - 1) / window)
    want = ([[1] * 2, [window] * 2] * n)[:len(strides)]          # 1, W, 1, W, ... with the last one capped by the end
    assert strides[:-1] == want[:-1] and strides[-1] == [n - sum(s[0] for s in strides[:-1])] * 2
    assert torch.equal(got, _sequential(eps_fn, x, sched))


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def test_the_gpu_fixture_stays_clear_of_its_threshold(tiny):
    cfg, sd = tiny
    f = FIXTURE
    sched = _schedule(f["steps"])
    _, strides, errs = po.sample(po.unet_eps(sd, cfg, sched), start(f["seeds"]), sched, f["window"], f["tolerance"])
    ratios = [e / f["tolerance"] ** 2 for it in errs for image in it for e in image]
    print(f"[picard host] fixture strides {strides}; err / tol^2 from {min(r for r in ratios if r > 0):.3g} to {max(ratios):.3g}")
    assert not [r for r in ratios if 0.5 <= r <= 2.0], ratios
    base, short = [0, 0], False
    for it in strides:
        for p, s in enumerate(it):
            base[p] += s
            short = short or (1 <= s < f["window"] and base[p] < f["steps"])
    assert any(s > 1 for it in strides for s in it) and short
    assert strides == [[1, 1], [1, 1], [3, 3], [1, 1]]


def test_the_uneven_pair_finishes_after_different_counts(tiny):
    cfg, sd = tiny
    f = UNEVEN
    sched = _schedule(f["steps"])
    _, strides, errs = po.sample(po.unet_eps(sd, cfg, sched), start(f["seeds"]), sched, f["window"], f["tolerance"])
    assert strides == [[1, 1], [3, 2], [0, 1]]
    near = [e / f["tolerance"] ** 2 for it in errs for image in it for e in image if 0.5 <= e / f["tolerance"] ** 2 <= 2.0]
    print(f"[picard host] uneven pair: err / tol^2 nearest the threshold: {sorted(near)}")
    assert all(abs(r - 1.0) >= 0.05 for r in near)          # 5 % from the threshold; fp32 moves an err by 1e-6 of itself


# ------------------------------------------------------------------------------------------------ surface
def _cpu_pipe(scheduler=None):
    from afldm_amd.models.unet_2d import UNet2DModel
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from oracle import configs as oc
    return MyLDMPipeline(None, UNet2DModel.from_config(oc.tiny_unet()), scheduler or ffhq_ddim_scheduler())


def test_signatures_and_defaults():
    from afldm_amd.engine import DenoiseEngine, PicardEngine
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    import afldm.pipelines.ldm_pipeline as alias
    assert alias.MyLDMPipeline.sample_parallel is MyLDMPipeline.sample_parallel
    sig = inspect.signature(MyLDMPipeline.sample_parallel_latents)
    assert list(sig.parameters)[1:8] == ["batch_size", "num_inference_steps", "window", "tolerance", "generator", "latents", "use_graph"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["batch_size"], d["num_inference_steps"], d["window"], d["tolerance"], d["generator"], d["latents"], d["use_graph"],
            d["eta"]) == (1, 50, 8, 0.1, None, None, True, 0.0)
    d = {k: v.default for k, v in inspect.signature(MyLDMPipeline.sample_parallel).parameters.items()}
    assert (d["window"], d["tolerance"], d["output_type"], d["return_dict"]) == (8, 0.1, "pil", True)
    assert issubclass(PicardEngine, DenoiseEngine) and PicardEngine.ONE_BRANCH and list(PicardEngine.UPDATES) == ["ddim"]
    d = {k: v.default for k, v in inspect.signature(PicardEngine.__init__).parameters.items()}
    assert (d["window"], d["tolerance"], d["steps_per_graph"]) == (8, 0.1, 5)


def test_refusals():
    from afldm_amd.engine import PicardEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    pipe = _cpu_pipe()
    with pytest.raises(NotImplementedError, match="eta"):
        pipe.sample_parallel_latents(num_inference_steps=4, eta=0.5)
    with pytest.raises(NotImplementedError, match="eta"):
        pipe.sample_parallel(num_inference_steps=4, eta=0.5, output_type="latent")
    for window in (0, -1, 2.5):
        with pytest.raises(ValueError, match="window"):
            pipe.sample_parallel_latents(num_inference_steps=4, window=window)
    with pytest.raises(ValueError, match="tolerance"):
        pipe.sample_parallel_latents(num_inference_steps=4, tolerance=-0.1)
    for use_graph in (True, False):
        with pytest.raises(RuntimeError, match="no CPU path"):
            pipe.sample_parallel_latents(num_inference_steps=4, window=2, use_graph=use_graph)
    dpm = _cpu_pipe(DPMSolverMultistepScheduler.from_config(ffhq_ddim_scheduler().config))
    with pytest.raises(NotImplementedError, match="DDIMScheduler"):
        dpm.sample_parallel_latents(num_inference_steps=4)
    for sched, kind in ((ffhq_ddim_scheduler().stochastic_schedule(4, 0.5), "sde"), (ffhq_ddim_scheduler().repaint_schedule(4, 0.0, 2, 2), "repaint"),
                        (dpm.scheduler.schedule(4), "dpm")):
        with pytest.raises(NotImplementedError, match=f"'{kind}'"):
            PicardEngine(pipe.unet, sched, 1, len(sched.timesteps))
    with pytest.raises(RuntimeError, match="no CPU path"):
        PicardEngine(pipe.unet, ffhq_ddim_scheduler().schedule(4), 1, 4)


def test_entry_points_are_bound_and_documented():
    from afldm_amd import _lib, build, ops
    names = ("afldm_picard_blocks", "afldm_picard_sweep", "afldm_picard_stride", "afldm_picard_slide")
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(ROOT, "afldm_amd", "csrc", "picard.hip")).read()
    for name in names:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name + "(" in hdr and name in doc
        assert 'extern "C" int ' + name + "(" in src
    assert "picard.hip" in build.SOURCES
    for f in ("picard_blocks", "picard_sweep", "picard_stride", "picard_slide"):
        assert callable(getattr(ops, f))
    # the workspace follows from the shape alone: 256 threads of 4 elements where a plane is whole groups of 4, else of 1
    assert (ops.picard_blocks(4, 16, 16), ops.picard_blocks(3, 5, 7), ops.picard_blocks(3, 64, 64), ops.picard_blocks(4, 32, 32)) == (1, 1, 12, 4)
    assert ops.picard_blocks(1, 1, 257) == 2
    x, y = torch.zeros(3, 1, 3, 5, 7), torch.zeros(2, 1, 3, 5, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.picard_sweep(x, torch.zeros(2, 5, 7, 3), y, torch.zeros(1, 2, 1), torch.ones(4, 4), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.picard_slide(x, y, torch.zeros(1, dtype=torch.int32))


def test_script_exists_and_parses_help():
    script = os.path.join(ROOT, "scripts", "sample_parallel_ffhq.py")
    assert os.path.exists(script)
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--ckpt", "--random-init", "--dtype", "--window", "--tolerance", "--timings", "--steps"):
        assert flag in r.stdout, flag
