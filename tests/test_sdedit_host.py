"""Image-to-image sampling (SDEdit with a change map), host side (no GPU): DDIMScheduler.sdedit_schedule - the reference's
get_timesteps, every coefficient row against its definition restated here, the thresholds, the draw pattern and the key - the
float64 restatement the GPU tests compare against (tests/sdedit_oracle.py) on its own invariants, the bindings' bookkeeping and
the argument validation of the pipeline entries."""
import inspect
import math
import os
import subprocess
import sys

import pytest
import torch

import sdedit_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


def sched(**kw):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    return DDIMScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)


def reference_timesteps(s, N, strength):
    """get_timesteps of the reference (video_equiv_editing_pipeline.py:320-328), restated."""
    s.set_timesteps(N)
    init = min(int(N * strength), N)
    t_start = max(N - init, 0)
    return [int(t) for t in s.timesteps][t_start:], N - t_start


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("N,strength,n", [(50, 0.58, 28), (50, 1.0, 50), (8, 0.5, 4), (50, 0.6, 30), (10, 0.99, 9), (3, 0.34, 1)])
def test_timesteps_are_the_references(N, strength, n):
    from afldm_amd.schedulers.schedule import KINDS, NOISE_SLOTS, ROW_WIDTH
    assert KINDS["sdedit"] == (12, 1, True) and ROW_WIDTH["sdedit"] == 12 and NOISE_SLOTS["sdedit"] == 1
    s = sched()
    sd = s.sdedit_schedule(N, strength)
    ts, count = reference_timesteps(sched(), N, strength)
    assert count == n and list(sd.timesteps) == ts and len(sd.rows) == n
    assert sd.kind == "sdedit" and sd.noise_dtype is None and sd.init_noise_sigma == 1.0
    ab0 = float(s.alphas_cumprod[ts[0]])
    assert s.sdedit_start(N, strength) == (math.sqrt(ab0), math.sqrt(1 - ab0))


def test_strength_that_runs_nothing_or_is_out_of_range_is_refused():
    for N, strength in ((50, 0.01), (8, 0.0), (8, 0.12), (8, -0.1), (8, 1.5), (8, math.nan)):
        with pytest.raises(ValueError):
            sched().sdedit_schedule(N, strength)
        with pytest.raises(ValueError):
            sched().sdedit_start(N, strength)
    with pytest.raises(NotImplementedError):
        sched(prediction_type="v_prediction").sdedit_schedule(8, 0.5)


@pytest.mark.parametrize("one", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_rows_are_the_definition(eta, one):
    for N, strength in ((8, 0.5), (50, 0.58), (6, 1.0)):
        s = sched(set_alpha_to_one=one)
        sd = s.sdedit_schedule(N, strength, eta)
        ts, n = reference_timesteps(sched(set_alpha_to_one=one), N, strength)
        for k, (t, row) in enumerate(zip(ts, sd.rows)):
            last = k == n - 1
            ab = float(s.alphas_cumprod[t])
            abn = float(s.final_alpha_cumprod) if last else float(s.alphas_cumprod[ts[k + 1]])
            assert row[:7] == s._reverse_row(ab, abn, eta)                               # float for float
            sigma = eta * math.sqrt((1 - abn) / (1 - ab) * (1 - ab / abn))
            assert row[:7] == (1 / math.sqrt(ab), -math.sqrt(1 - ab) / math.sqrt(ab), -INF, INF, math.sqrt(abn),
                               math.sqrt(max(1 - abn - sigma * sigma, 0.0)), sigma)
            assert row[7:9] == ((1.0, 0.0) if last else (math.sqrt(abn), math.sqrt(1 - abn)))
            assert row[9] == (n - 1 - k) / n and row[10:] == (0.0, 0.0)
        # the draws: z_u where sigma != 0, as panorama_schedule draws
        assert sd.draws == tuple(r[6] != 0.0 for r in sd.rows)
        assert [sd.slots(k) for k in range(n)] == [(0,) if r[6] != 0.0 else () for r in sd.rows]
        if eta == 0.0:
            assert not any(sd.draws)
        else:
            assert all(sd.draws[:-1]) and sd.draws[-1] == (not one)                      # alpha_to_one: the last sigma is 0
    # clip_sample: the bounds reach the row (the reverse step is repaint_schedule's)
    row = sched(clip_sample=True).sdedit_schedule(8, 0.5).rows[0]
    assert row[2:4] == (-1.0, 1.0)


def test_thresholds():
    sd = sched().sdedit_schedule(8, 0.5)
    assert [r[9] for r in sd.rows] == [0.75, 0.5, 0.25, 0.0]
    assert [float(v) for v in sd.table("cpu")[:, 9]] == [0.75, 0.5, 0.25, 0.0]           # exact in fp32 too
    for N, strength in ((50, 0.58), (50, 1.0), (7, 0.9)):
        rows = sched().sdedit_schedule(N, strength).rows
        n = len(rows)
        thr = [r[9] for r in rows]
        assert thr[0] == 1 - 1 / n < 1.0 and thr[-1] == 0.0 and all(a > b for a, b in zip(thr, thr[1:]))
        assert rows[-1][7:9] == (1.0, 0.0)


def test_key_and_caching():
    from afldm_amd.schedulers import schedule
    a = sched().sdedit_schedule(8, 0.5, 0.3)
    assert sched().sdedit_schedule(8, 0.5, 0.3) is a                                     # one Schedule per key
    assert sched().sdedit_schedule(8, 0.55, 0.3) is a                                    # int(8 * 0.55) = 4 too: the same rows
    settings = dict(a.key[1])
    assert (settings["_sdedit_steps"], settings["_sdedit_strength"], settings["_sdedit_eta"]) == ("8", "4", "0.3")
    assert a.key[0] == "DDIMScheduler" and schedule._MADE[a.key] is a
    others = [sched().sdedit_schedule(8, 0.5, 0.0), sched().sdedit_schedule(8, 0.75, 0.3), sched().sdedit_schedule(4, 1.0, 0.3),
              sched(beta_end=0.02).sdedit_schedule(8, 0.5, 0.3)]
    assert len({o.key for o in others} | {a.key}) == 5
    assert len(others[2].timesteps) == 4 and others[2].timesteps != a.timesteps          # n = 4 of N = 4: other timesteps, other key
    # the schedules of the other kinds are left alone
    rp = sched().repaint_schedule(6, 0.0, 2, 2)
    assert rp.kind == "repaint" and not any(k.startswith("_sdedit") for k, _ in rp.key[1])


# ------------------------------------------------------------------------------------------------ oracle
def _eps(x, t):
    return torch.sin(x + float(t))


def _loop_inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    orig = torch.randn(2, 3, 5, 5, generator=g, dtype=torch.float64)
    z = torch.randn(2, 3, 5, 5, generator=g, dtype=torch.float64)
    cmap = torch.randint(0, 5, (2, 1, 5, 5), generator=g).double() / 4                   # {0, 1/4, 1/2, 3/4, 1}
    cmap[0, 0, 0] = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0], dtype=torch.float64)       # every level is there
    return orig, z, cmap


@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_oracle_loop_properties(eta):
    s = sched()
    sd = s.sdedit_schedule(8, 0.5, eta)
    start = s.sdedit_start(8, 0.5)
    orig, z, cmap = _loop_inputs()
    n = len(sd.rows)
    assert n == 4
    g = torch.Generator().manual_seed(9)
    noises = [torch.randn(orig.shape, generator=g, dtype=torch.float64) for _ in range(n)]
    it = iter(noises)
    trace = []
    out = so.sample(_eps, orig, cmap, z, sd, start, draw=lambda: next(it), trace=trace)
    assert len(trace) == n and torch.equal(out, trace[-1]) and out.dtype == torch.float64
    assert len(list(it)) == n - sum(len(sd.slots(k)) for k in range(n))                  # one draw per evaluation that draws
    full = cmap.expand_as(orig)
    # change value 0: the original, bit for bit
    assert torch.equal(out[full == 0], orig[full == 0]) and int((full == 0).sum()) > 0
    # change value 1: the plain truncated reverse loop from x_start (the elements are independent under eps = sin(x + t))
    it = iter(noises)
    plain = so.sample_plain(_eps, so.x_start(orig, z, start), sd, draw=lambda: next(it))
    assert torch.equal(out[full == 1], plain[full == 1]) and int((full == 1).sum()) > 0
    assert not torch.equal(out[full == 0.5], plain[full == 0.5])
    # a value c: on the original's noised trajectory after every evaluation k with c <= thr_k, off it afterwards
    rows = so.rows_of(sd)
    for c in (0.0, 0.25, 0.5, 0.75, 1.0):
        sel = full == c
        for k in range(n):
            k0, k1, thr = rows[k][7], rows[k][8], rows[k][9]
            held = (k0 * orig + k1 * z)[sel]
            if c <= thr:
                assert torch.equal(trace[k][sel], held), (c, k)
            else:
                assert (trace[k][sel] != held).all(), (c, k)
    # the start is the update under the start row, whatever x and eps hold
    nan = torch.full_like(orig, math.nan)
    assert torch.equal(so.sdedit_step(nan, nan, orig, torch.zeros_like(orig), z, None, so.f32(so.start_row(*start))),
                       so.x_start(orig, z, start))


def test_oracle_step_selects():
    """A NaN on the side that is not selected does not reach the result; a NaN in the change map is generated; an unused noise
    is not looked at."""
    g = torch.Generator().manual_seed(4)
    x, e, orig, z, zu = [torch.randn(1, 2, 3, 4, generator=g, dtype=torch.float64) for _ in range(5)]
    cmap = torch.tensor([0.0, 0.5, 0.75, math.nan]).reshape(1, 1, 1, 4).expand(1, 1, 3, 4).double()
    row = so.f32((1.25, -0.75, -INF, INF, 0.9, 0.3, 0.2, 0.8, 0.6, 0.5))
    want_held = row[7] * orig + row[8] * z
    want_xp = row[4] * (row[0] * x + row[1] * e) + row[5] * e + row[6] * zu
    out = so.sdedit_step(x, e, orig, cmap, z, zu, row)
    assert torch.equal(out[..., :2], want_held[..., :2]) and torch.equal(out[..., 2:], want_xp[..., 2:])
    xn, en = x.clone(), e.clone()
    xn[..., 0], en[..., 1] = math.nan, math.inf
    assert torch.equal(so.sdedit_step(xn, en, orig, cmap, z, zu, row)[..., :2], want_held[..., :2])
    row0 = so.f32((1.25, -0.75, -INF, INF, 0.9, 0.3, 0.0, 1.0, 0.0, 0.5))
    out = so.sdedit_step(x, e, orig, cmap, torch.full_like(z, math.nan), None, row0)
    assert torch.isfinite(out).all() and torch.equal(out[..., :2], orig[..., :2])


# ------------------------------------------------------------------------------------------------ bindings
def test_entry_points_are_bound_and_documented():
    from afldm_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(ROOT, "afldm_amd", "csrc", "sdedit.hip")).read()
    for name in ("afldm_sdedit_step", "afldm_sdedit_step_flat"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name + "(" in hdr and name in doc
        assert 'extern "C" int ' + name + "(" in src
    assert "sdedit.hip" in build.SOURCES
    # no CPU path
    x, m = torch.zeros(1, 4, 4, 4), torch.ones(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sdedit_step(x, x.permute(0, 2, 3, 1).contiguous(), x, m, x, None, torch.zeros(12), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sdedit_step_flat(x, x, x, x, None, None, (1.0, 0.0, -1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.5))


def test_engine_and_pipeline_surface():
    from afldm_amd import engine
    from afldm_amd.engine import DenoiseEngine, SDEditEngine
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    import afldm.pipelines.ldm_pipeline as alias
    assert alias.MyLDMPipeline.img2img is MyLDMPipeline.img2img and alias.MyLDMPipeline.img2img_latents is MyLDMPipeline.img2img_latents
    assert issubclass(SDEditEngine, DenoiseEngine) and not SDEditEngine.ONE_BRANCH
    assert list(SDEditEngine.UPDATES) == ["sdedit"]
    others = [c for c in vars(engine).values() if inspect.isclass(c) and issubclass(c, DenoiseEngine) and c is not SDEditEngine]
    assert len(others) >= 8
    for other in others:
        assert "sdedit" not in other.UPDATES, other
    sig = inspect.signature(MyLDMPipeline.img2img_latents)
    assert list(sig.parameters)[1:] == ["orig_latents", "strength", "change_map", "num_inference_steps", "eta", "generator", "noise",
                                        "use_graph"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["strength"], d["change_map"], d["num_inference_steps"], d["eta"], d["generator"], d["noise"], d["use_graph"]) == (
        0.6, None, 50, 0.0, None, None, True)
    sig = inspect.signature(MyLDMPipeline.img2img)
    assert list(sig.parameters)[1:4] == ["image", "strength", "change_map"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["strength"], d["change_map"], d["composite"], d["output_type"], d["return_dict"]) == (0.6, None, True, "pil", True)
    for f in (I2SBLDMPipeline.img2img_latents, I2SBLDMPipeline.img2img):
        with pytest.raises(NotImplementedError):
            f(object(), torch.zeros(1, 4, 32, 32))


class _FakeUnet:
    dtype, device = torch.float32, torch.device("cpu")

    class config:
        in_channels, sample_size = 4, 8


class _FakeVae:
    dtype = torch.float32

    class config:
        block_out_channels, scaling_factor = (8, 8, 8), 0.5


def _pipe(scheduler=None, vae=None):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    pipe = MyLDMPipeline(vae, _FakeUnet(), scheduler or sched())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def test_argument_validation(monkeypatch):
    from afldm_amd import engine
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    monkeypatch.setattr(engine, "SDEditEngine", lambda *a, **k: pytest.fail("no engine before the arguments are checked"))
    z0, m = torch.zeros(2, 4, 8, 8), torch.ones(2, 1, 8, 8)
    pipe = _pipe()
    for bad_z, bad_m, noise in [(torch.zeros(2, 3, 8, 8), m, None), (torch.zeros(2, 4, 8, 4), m, None), (torch.zeros(4, 8, 8), m, None),
                                (z0, torch.ones(2, 4, 8, 8), None), (z0, torch.ones(3, 1, 8, 8), None), (z0, torch.ones(2, 1, 4, 4), None),
                                (z0, torch.ones(1, 8, 8), None), (z0, m, torch.zeros(1, 4, 8, 8))]:
        with pytest.raises(ValueError):
            pipe.img2img_latents(bad_z, 0.5, bad_m, num_inference_steps=8, noise=noise)
    for strength in (-0.1, 1.01, 0.1):                                                   # out of range; int(8 * 0.1) = 0: nothing runs
        with pytest.raises(ValueError):
            pipe.img2img_latents(z0, strength, m, num_inference_steps=8)
    # no VAE: img2img refuses and points at the latent entry
    with pytest.raises(NotImplementedError, match="img2img_latents"):
        pipe.img2img(torch.zeros(2, 3, 32, 32))
    # with one: shapes and the strength are checked before anything touches the GPU (the fake VAE cannot encode)
    vp = _pipe(vae=_FakeVae())
    for img, cm in [(torch.zeros(2, 3, 32, 16), None), (torch.zeros(2, 1, 32, 32), None), (torch.zeros(2, 3, 32, 32), torch.ones(1, 1, 8, 8)),
                    (torch.zeros(2, 3, 32, 32), torch.ones(3, 1, 32, 32)), (torch.zeros(2, 3, 32, 32), torch.ones(2, 3, 32, 32))]:
        with pytest.raises(ValueError):
            vp.img2img(img, 0.5, cm)
    with pytest.raises(ValueError):
        vp.img2img(torch.zeros(2, 3, 32, 32), 1.5)
    # DPM-Solver: refused by name from both entries
    dp = _pipe(DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG), vae=_FakeVae())
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        dp.img2img_latents(z0, 0.5, m)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        dp.img2img(torch.zeros(2, 3, 32, 32))


def test_script_parses_its_options():
    import importlib.util
    script = os.path.join(ROOT, "scripts", "img2img_ffhq.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--image", "--strength", "--change-map", "--ramp", "--eta", "--random-init"):
        assert flag in r.stdout, flag
    spec = importlib.util.spec_from_file_location("img2img_ffhq", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["--image", "a.png", "--strength", "0.4", "--change-map", "m.png", "--eta", "0.5", "--seed", "7"])
    assert (a.image, a.strength, a.change_map, a.ramp, a.eta, a.seed) == ("a.png", 0.4, "m.png", False, 0.5, 7)
    assert mod.parse_args(["--random-init", "--ramp"]).ramp
    for bad in ([], ["--random-init", "--strength", "1.5"], ["--random-init", "--strength", "0.01"],
                ["--random-init", "--ramp", "--change-map", "m.png"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    ramp = mod.ramp_map(16)
    assert tuple(ramp.shape) == (1, 1, 16, 16) and float(ramp[0, 0, 3, 0]) == 0.0 and float(ramp[0, 0, 3, -1]) == 1.0
    assert (ramp[..., 1:] > ramp[..., :-1]).all()
