"""Schedule (afldm_amd/schedulers/schedule.py), host side: the fp32 table of every producer is bit-equal to the table its
scheduler-shaped predecessor built - restated here, each in the spelling it had (torch.tensor(rows, float32) for the DDIM-form
rows, torch.tensor(rows, float64).to(float32) for the 8-wide ones) - and the key tells apart what must not share a graph."""
import dataclasses

import pytest
import torch

from afldm_amd.configs import FFHQ_DDIM_CONFIG
from afldm_amd.schedulers.schedule import Schedule

I2SB_CFG = {k: v for k, v in FFHQ_DDIM_CONFIG.items() if k != "set_alpha_to_one"}


def _check(sched, kind, timesteps, want, draws=None):
    assert isinstance(sched, Schedule) and sched.kind == kind
    assert sched.timesteps == tuple(timesteps) and all(type(t) is int for t in sched.timesteps)
    assert sched.draws == (tuple(draws) if draws is not None else (False,) * len(timesteps))
    table = sched.table("cpu")
    assert table.dtype == torch.float32 and tuple(table.shape) == (len(timesteps), 4 if kind == "ddim" else 8)
    assert torch.equal(table, want)
    hash(sched.key)
    with pytest.raises(dataclasses.FrozenInstanceError):
        sched.rows = ()


@pytest.mark.parametrize("spacing", ["leading", "trailing", "linspace"])
@pytest.mark.parametrize("steps", [1, 7, 50])
def test_ddim_tables(spacing, steps):
    from afldm_amd.schedulers.ddim import DDIMScheduler
    s = DDIMScheduler.from_config(dict(FFHQ_DDIM_CONFIG, timestep_spacing=spacing))
    sched = s.schedule(steps)
    ts = s._timesteps_host
    _check(sched, "ddim", ts, torch.tensor([s.coefficients(t) for t in ts], dtype=torch.float32))
    assert torch.equal(s.coefficient_table("cpu"), sched.table("cpu")) and sched.init_noise_sigma == 1.0
    for eta in (0.3, 1.0):
        sde = s.stochastic_schedule(steps, eta)
        want = torch.tensor([s.sde_coefficients(t, eta) for t in ts], dtype=torch.float64).to(torch.float32)
        _check(sde, "sde", ts, want, [True] * steps)
        assert sde.noise_dtype is None and sde.key != sched.key and sde.key != s.stochastic_schedule(steps, 0.5).key
    assert sched.key == DDIMScheduler.from_config(s.config).schedule(steps).key != s.schedule(steps + 1).key


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("algo,final", [("dpmsolver++", "zero"), ("dpmsolver", "sigma_min")])
@pytest.mark.parametrize("steps", [3, 20])
def test_dpm_tables(order, algo, final, steps):
    from afldm_amd.schedulers.ddim import DDIMScheduler
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, solver_order=order, algorithm_type=algo, final_sigmas_type=final)
    sched = s.schedule(steps)
    want = torch.tensor(s._rows, dtype=torch.float64).to(torch.float32)
    _check(sched, "dpm", s._timesteps_host, want)
    assert torch.equal(s.coefficient_table("cpu"), want) and s.schedule().key == sched.key
    # same config keys, another class: another key
    assert sched.key[0] == "DPMSolverMultistepScheduler" != DDIMScheduler.from_config(FFHQ_DDIM_CONFIG).schedule(steps).key[0]
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler().schedule()


@pytest.mark.parametrize("steps", [2, 10, 100])
def test_i2sb_tables(steps):
    from afldm_amd.schedulers.i2sb import I2SBScheduler
    s = I2SBScheduler.from_config(I2SB_CFG)
    ode = s.ode_schedule(steps)
    ts = s._timesteps_host[:steps - 1]
    assert len(ts) == steps - 1
    _check(ode, "ddim", ts, torch.tensor([s.ode_coefficients(t) for t in ts], dtype=torch.float32).reshape(-1, 4))
    keys = {ode.key}
    for is_ode, clip in [(False, False), (False, True), (True, True)]:
        c = I2SBScheduler.from_config(dict(I2SB_CFG, clip_sample=clip))
        assert (c.ode_schedule(steps) is None) == clip
        sde = c.bridge_schedule(steps, is_ode)
        want = torch.tensor([c.sde_coefficients(t, is_ode) for t in ts], dtype=torch.float64).to(torch.float32).reshape(-1, 8)
        _check(sde, "sde", ts, want, [t > 0 and not is_ode for t in ts])
        assert sde.noise_dtype == torch.float32
        keys.add(sde.key)
    assert len(keys) == 4                                             # the ODE and SDE bridges never share an engine


def test_inversion_table():
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = MyLDMPipeline.__new__(MyLDMPipeline)
    pipe.scheduler = ffhq_ddim_scheduler()
    pipe.scheduler.set_timesteps(9)
    rows = pipe._inversion_rows()
    inv = pipe.inversion_schedule()
    _check(inv, "ddim", [t for t, _ in rows], torch.tensor([c for _, c in rows], dtype=torch.float32))
    assert inv.key != pipe.scheduler.schedule(9).key
    pipe.scheduler.set_timesteps(8)
    assert pipe.inversion_schedule().key != inv.key


def test_engine_rejects_unknown_kind_and_wrong_length():
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler

    class Unet:
        dtype, device = torch.float32, torch.device("cuda")

    sched = ffhq_ddim_scheduler().schedule(4)
    with pytest.raises(NotImplementedError, match="update_kind 'heun'"):
        DenoiseEngine(Unet(), dataclasses.replace(sched, kind="heun"), 1, 4)
    with pytest.raises(ValueError):
        DenoiseEngine(Unet(), sched, 1, 5)
