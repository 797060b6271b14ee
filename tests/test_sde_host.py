"""Stochastic samplers on the graph engine, host side: the (p, q, lo, hi, a, b, d, c) rows of DDIMScheduler.stochastic_schedule
and I2SBScheduler.bridge_schedule against float64 restatements of diffusers' DDIMScheduler.step(eta) and the reference
I2SB step, the rows applied with the schedules' own draws against the oracle schedulers' loops (same generator, same
generator state afterwards), and the pipelines' routing.  No GPU needed."""
import itertools
import math

import numpy as np
import pytest
import torch

from afldm_amd.configs import FFHQ_DDIM_CONFIG

I2SB_CFG = {k: v for k, v in FFHQ_DDIM_CONFIG.items() if k != "set_alpha_to_one"}


def apply_row(row, x, e, z):
    """afldm_sde_step's update in float64: x0 = clamp(p x + q e, lo, hi); x_out = a x + b x0 + d e + c z."""
    p, q, lo, hi, a, b, d, c = row
    x0 = (p * x + q * e).clamp(lo, hi)
    return a * x + b * x0 + d * e + c * z


def rel_rms(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def _data(seed, shape=(2, 4, 8, 8)):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(3)]


# ------------------------------------------------------------------------------------------------ DDIM, eta != 0
def ref_ddim_step(ac, final, T, n, t, x, e, z, eta):
    """diffusers DDIMScheduler.step (epsilon prediction, no clip, eta) restated in float64 from the fp32 alphas_cumprod."""
    prev_t = t - T // n
    a_t = float(ac[t])
    a_prev = float(ac[prev_t]) if prev_t >= 0 else final
    x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
    variance = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
    std = eta * variance ** 0.5
    return a_prev ** 0.5 * x0 + (1 - a_prev - std ** 2) ** 0.5 * e + std * z


@pytest.mark.parametrize("eta,spacing,one,steps", list(itertools.product(
    [0.3, 1.0], ["leading", "trailing", "linspace"], [True, False], [1, 8, 50])))
def test_ddim_rows_vs_diffusers_restatement(eta, spacing, one, steps):
    from afldm_amd.schedulers.ddim import DDIMScheduler
    cfg = dict(FFHQ_DDIM_CONFIG, timestep_spacing=spacing, set_alpha_to_one=one)
    s = DDIMScheduler.from_config(cfg)
    sde = s.stochastic_schedule(steps, eta)
    assert sde.update_kind == "sde" and len(sde.rows) == steps and sde.draws == (True,) * steps
    assert sde.noise_dtype is None                                     # the model's dtype, as step() draws
    assert sde._timesteps_host == s._timesteps_host and sde.config._ddim_eta == eta
    betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, 0).double()
    final = 1.0 if one else float(ac[0])
    x, e, z = _data(steps)
    for t, row in zip(sde._timesteps_host, sde.rows):
        assert row[2] == -math.inf and row[3] == math.inf and row[4] == 0.0
        want = ref_ddim_step(ac, final, 1000, steps, t, x, e, z, eta)
        got = apply_row(row, x, e, z)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), (t, float((got - want).abs().max()))
    # the last step (prev_t < 0 for every spacing here) has sigma = 0 when a_prev = 1 or a_prev = a_t (t = 0), and still draws
    t_last = s._timesteps_host[-1]
    assert t_last - 1000 // steps < 0 and (sde.rows[-1][7] == 0.0) == (one or t_last == 0)
    table = sde.coefficient_table("cpu")
    assert table.dtype == torch.float32 and tuple(table.shape) == (steps, 8)
    assert torch.equal(table, torch.tensor(sde.rows, dtype=torch.float64).float())


def test_ddim_stochastic_schedule_keeps_raising_on_clip_sample():
    from afldm_amd.schedulers.ddim import DDIMScheduler
    with pytest.raises(NotImplementedError):
        DDIMScheduler.from_config(dict(FFHQ_DDIM_CONFIG, clip_sample=True)).stochastic_schedule(10, 0.5)


# ------------------------------------------------------------------------------------------------ I2SB bridge
def ref_i2sb_step(std_fwd, t, prev_t, x, e, z, is_ode, clip):
    """Reference i2sb_scheduler.py:382-459 (epsilon prediction) in float64 from the fp32 std_fwd table."""
    s, sp = float(std_fwd[t]), float(std_fwd[prev_t])
    sd = (s * s - sp * sp) ** 0.5
    x0 = x - s * e
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    denom = sp * sp + sd * sd
    mu_x0, mu_xt, var = sd * sd / denom, sp * sp / denom, sp * sp * sd * sd / denom
    prev = mu_x0 * x0 + mu_xt * x
    if t > 0 and not is_ode:
        prev = prev + z * var ** 0.5
    return prev


@pytest.mark.parametrize("is_ode,clip", list(itertools.product([False, True], [False, True])))
@pytest.mark.parametrize("steps", [2, 10, 100])
def test_i2sb_rows_vs_reference_step(is_ode, clip, steps):
    from afldm_amd.schedulers.i2sb import I2SBScheduler
    s = I2SBScheduler.from_config(dict(I2SB_CFG, clip_sample=clip))
    sde = s.bridge_schedule(steps, is_ode)
    assert sde.update_kind == "sde" and len(sde.rows) == steps - 1 and sde.noise_dtype == torch.float32
    assert sde._timesteps_host == s._timesteps_host[:steps - 1]
    assert sde.draws == tuple(t > 0 and not is_ode for t in sde._timesteps_host)
    x, e, z = _data(steps)
    x = 1.5 * x                                                        # so that x0 crosses the clip bounds
    for t, row in zip(sde._timesteps_host, sde.rows):
        p, q, lo, hi, a, b, d, c = row
        assert p == 1.0 and d == 0.0 and q == -float(s.std_fwd[t])
        assert (lo, hi) == ((-1.0, 1.0) if clip else (-math.inf, math.inf))
        assert (c == 0.0) == is_ode
        want = ref_i2sb_step(s.std_fwd, t, s.previous_timestep(t), x, e, z, is_ode, clip)
        assert torch.allclose(apply_row(row, x, e, z), want, rtol=1e-12, atol=1e-12), t
    if clip:
        assert ((x - float(s.std_fwd[sde._timesteps_host[0]]) * e).abs() > 1).any()


def test_i2sb_rows_at_t0_and_clip_range():
    from afldm_amd.schedulers.i2sb import I2SBScheduler
    s = I2SBScheduler.from_config(dict(I2SB_CFG, clip_sample=True, clip_sample_range=2.5, steps_offset=0))
    s.set_timesteps(10)
    assert s._timesteps_host[-1] == 0
    for is_ode in (False, True):
        row = s.sde_coefficients(0, is_ode)
        assert row[7] == 0.0 and row[2:4] == (-2.5, 2.5) and row[0] == 1.0
    assert s.sde_coefficients(100, False)[7] > 0 and s.sde_coefficients(100, True)[7] == 0.0
    # the unclipped ODE rows are the same update as ode_coefficients' linear form
    u = I2SBScheduler.from_config(I2SB_CFG)
    u.set_timesteps(10)
    x, e, z = _data(3)
    for t in u._timesteps_host[:9]:
        c0, c1, c2, c3 = u.ode_coefficients(t)
        lin = c2 * (x - c1 * e) / c0 + c3 * e
        assert torch.allclose(apply_row(u.sde_coefficients(t, True), x, e, z), lin, rtol=1e-6, atol=1e-6)
    # ode_schedule is unchanged: None under clip_sample
    assert s.ode_schedule(10) is None


# ------------------------------------------------------------------------------------------------ draws vs the oracle loops
def _model(x, t):
    """A stand-in for the UNet: any deterministic function of (x, t)."""
    return torch.tanh(0.7 * x + 1e-3 * t)


@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_ddim_rows_and_draws_reproduce_oracle_loop(eta):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from oracle import ddim as od
    x0 = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    o = od.DDIM()
    o.set_timesteps(12)
    go = torch.Generator().manual_seed(7)
    ref = x0.clone()
    for t in o.timesteps:
        ref = o.step(_model(ref, int(t)), t, ref, eta=eta, generator=go)
    sde = ffhq_ddim_scheduler().stochastic_schedule(12, eta)
    gs = torch.Generator().manual_seed(7)
    draw = sde.drawer(gs, tuple(x0.shape), torch.device("cuda"), torch.float32)
    x = x0.double()
    for t, row, d in zip(sde._timesteps_host, sde.rows, sde.draws):
        z = draw().double() if d else torch.zeros_like(x)
        x = apply_row(row, x, _model(x.float(), t).double(), z)
    assert torch.equal(gs.get_state(), go.get_state())
    err = rel_rms(x, ref)
    assert err <= 1e-6, err                                            # the oracle runs in fp32


@pytest.mark.parametrize("is_ode,clip", list(itertools.product([False, True], [False, True])))
def test_i2sb_rows_and_draws_reproduce_oracle_loop(is_ode, clip):
    from afldm_amd.schedulers.i2sb import I2SBScheduler
    from oracle import i2sb as oi
    x0 = 1.2 * torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(2))
    o = oi.I2SB(clip_sample=clip)
    o.set_timesteps(20)
    go = torch.Generator().manual_seed(9)
    ref = x0.clone()
    for t in o.timesteps[:19]:
        ref = o.step(_model(ref, int(t)), t, ref, is_ode=is_ode, generator=go)
    sde = I2SBScheduler.from_config(dict(I2SB_CFG, clip_sample=clip)).bridge_schedule(20, is_ode)
    assert sde._timesteps_host == [int(t) for t in o.timesteps[:19]]
    gs = torch.Generator().manual_seed(9)
    draw = sde.drawer(gs, tuple(x0.shape), torch.device("cuda"), torch.bfloat16)
    x = x0.double()
    for t, row, d in zip(sde._timesteps_host, sde.rows, sde.draws):
        z = draw() if d else torch.zeros_like(x)
        assert z.dtype in (torch.float32, torch.float64)                # I2SB draws in fp32 whatever the model dtype
        x = apply_row(row, x, _model(x.float(), t).double(), z.double())
    assert torch.equal(gs.get_state(), go.get_state())
    err = rel_rms(x, ref)
    assert err <= 1e-6, err                                            # the oracle runs in fp32


def test_drawer_devices_and_generator_lists(monkeypatch):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    sde = ffhq_ddim_scheduler().stochastic_schedule(4, 1.0)
    gens = [torch.Generator().manual_seed(i) for i in range(3)]
    z = sde.drawer(gens, (3, 4, 8, 8), torch.device("cuda"), torch.bfloat16)()
    assert z.device.type == "cpu" and z.dtype == torch.bfloat16         # CPU generators: drawn on the host, staged by the engine
    for i in range(3):
        assert torch.equal(z[i:i + 1], torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(i), dtype=torch.bfloat16))
    calls = []
    monkeypatch.setattr(type(sde), "draw_noise", lambda self, shape, gen, device, dt: calls.append(device))
    sde.drawer(None, (1, 4, 8, 8), torch.device("cuda"), torch.float32)()
    assert calls == [torch.device("cuda")]                              # no generator: the device's default generator


# ------------------------------------------------------------------------------------------------ pipeline routing
class _FakeUnet:
    dtype, device = torch.float32, torch.device("cpu")

    class config:
        in_channels, sample_size = 4, 8

    def __call__(self, x, t):
        class Out:
            sample = torch.zeros_like(x)
        return Out()


class _CudaLike:
    """Stands for a CUDA latent tensor on a machine without one: the graph route only looks at is_cuda / shape / device / dtype."""
    is_cuda, dtype, device = True, torch.float32, torch.device("cuda")

    def __init__(self, shape):
        self.shape = torch.Size(shape)

    def to(self, *a, **k):
        return self


def _fake_engine(seen):
    class Engine:
        def __init__(self, unet, sched, batch, steps, use_graph):
            self.scheduler, self.steps = sched, steps
            seen.append(("init", getattr(sched, "update_kind", "ddim"), batch, steps, use_graph))

        def run(self, latents, draw=None):
            seen.append(("run", draw is not None))
            if draw is not None:
                for d in self.scheduler.draws:
                    if d:
                        draw()
            return latents
    return Engine


def test_ldm_pipeline_routes_eta_to_the_sde_engine(monkeypatch):
    from afldm_amd import engine
    from afldm_amd.pipelines import ldm_pipeline
    from afldm_amd.schedulers.ddim import DDIMScheduler, ffhq_ddim_scheduler
    seen, steps_called = [], []
    monkeypatch.setattr(engine, "DenoiseEngine", _fake_engine(seen))
    monkeypatch.setattr(DDIMScheduler, "step", lambda self, e, t, x, eta=0.0, generator=None, **k: steps_called.append(eta) or
                        type("O", (), {"prev_sample": x})())
    pipe = ldm_pipeline.MyLDMPipeline(None, _FakeUnet(), ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(5)
    pipe(latents=torch.zeros(2, 4, 8, 8), num_inference_steps=6, eta=0.7, generator=g, output_type="latent")
    assert seen == [("init", "sde", 2, 6, True), ("run", True)] and steps_called == []
    # the engine drew 6 steps from the caller's generator, on the host
    want = torch.Generator().manual_seed(5)
    for _ in range(6):
        torch.randn(2, 4, 8, 8, generator=want)
    assert torch.equal(g.get_state(), want.get_state())
    (key,) = pipe._engines
    assert "_ddim_eta" in dict(key[6]) and dict(key[6])["_ddim_eta"] == "0.7"
    # another eta: another engine; the same eta again: the cached one
    pipe(latents=torch.zeros(2, 4, 8, 8), num_inference_steps=6, eta=0.3, output_type="latent")
    pipe(latents=torch.zeros(2, 4, 8, 8), num_inference_steps=6, eta=0.3, output_type="latent")
    assert [s for s in seen if s[0] == "init"] == [("init", "sde", 2, 6, True)] * 2
    # use_graph=False: the eager loop, unchanged
    seen.clear()
    pipe(latents=torch.zeros(2, 4, 8, 8), num_inference_steps=6, eta=0.7, output_type="latent", use_graph=False)
    assert seen == [] and steps_called == [0.7] * 6
    # eta = 0: the deterministic engine
    pipe(latents=torch.zeros(2, 4, 8, 8), num_inference_steps=6, output_type="latent")
    assert seen == [("init", "ddim", 2, 6, True), ("run", False)]


def test_i2sb_pipeline_routes_stochastic_and_clipped_bridges(monkeypatch):
    from afldm_amd import engine
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    from afldm_amd.schedulers.i2sb import I2SBScheduler
    seen = []
    monkeypatch.setattr(engine, "DenoiseEngine", _fake_engine(seen))
    for is_ode, clip in [(False, True), (False, False), (True, True)]:
        seen.clear()
        pipe = I2SBLDMPipeline(None, _FakeUnet(), I2SBScheduler.from_config(dict(I2SB_CFG, clip_sample=clip)))
        pipe.set_progress_bar_config(disable=True)
        g = torch.Generator().manual_seed(3)
        pipe._bridge(_CudaLike((2, 4, 8, 8)), 10, is_ode, g)
        pipe._bridge(_CudaLike((2, 4, 8, 8)), 10, is_ode, g)
        assert seen == [("init", "sde", 2, 9, True), ("run", True), ("run", True)], (is_ode, clip)
        assert "_ode_engines" not in pipe.__dict__ and len(pipe._sde_engines) == 1
        want = torch.Generator().manual_seed(3)
        for _ in range(0 if is_ode else 2 * 9):
            torch.randn(2, 4, 8, 8, generator=want)
        assert torch.equal(g.get_state(), want.get_state())
    # the unclipped ODE keeps its own engine
    seen.clear()
    pipe = I2SBLDMPipeline(None, _FakeUnet(), I2SBScheduler.from_config(I2SB_CFG))
    pipe._bridge(_CudaLike((2, 4, 8, 8)), 10, True, None)
    assert seen == [("init", "ddim", 2, 9, True), ("run", False)] and "_sde_engines" not in pipe.__dict__
    # latent_dtype=None and use_graph=False keep the eager loop: its first UNet call is the fake's marker
    class Eager(Exception):
        pass

    class EagerUnet(_FakeUnet):
        def __call__(self, x, t):
            raise Eager
    seen.clear()
    clip = I2SBLDMPipeline(None, EagerUnet(), I2SBScheduler.from_config(dict(I2SB_CFG, clip_sample=True)))
    clip.set_progress_bar_config(disable=True)
    for kw in (dict(use_graph=False), dict(latent_dtype=None)):
        with pytest.raises(Eager):
            clip._bridge(_CudaLike((2, 4, 8, 8)), 10, False, None, **kw)
    assert seen == [] and "_sde_engines" not in clip.__dict__
