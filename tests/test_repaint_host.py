"""RePaint inpainting, host side (no GPU): DDIMScheduler.repaint_schedule - the evaluation sequence of diffusers'
RePaintScheduler.set_timesteps, every coefficient row against a float64 restatement from alphas_cumprod, the draw pattern and
the key - the "sde" schedules it must leave alone, argument validation of the pipeline entries, and the ops' refusal of CPU
tensors."""
import math

import pytest
import torch

# (N, jump_length, jump_n_sample) -> the evaluated indices (N - 1 = the noisiest timestep)
SEQUENCES = {
    (6, 2, 2): [5, 4, 3, 2, 3, 2, 1, 0, 1, 0],
    (8, 3, 2): [7, 6, 5, 4, 3, 5, 4, 3, 2, 1, 0, 2, 1, 0],
    (5, 1, 3): [4, 3, 3, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0],
    (6, 3, 2): [5, 4, 3, 2, 1, 0, 2, 1, 0],
    (4, 2, 1): [3, 2, 1, 0],
}


def sched(**kw):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    return DDIMScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)


def want_rows(s, n, ev, eta, bound=math.inf):
    """The rows of the issue's definition in float64, from the scheduler's fp32 alphas_cumprod."""
    s.set_timesteps(n)
    g = [int(t) for t in s.timesteps]
    ac = s.alphas_cumprod.double()

    def level(t):
        return float(ac[g[n - 1 - t]]) if t >= 0 else float(s.final_alpha_cumprod)
    rows = []
    for i, t in enumerate(ev):
        a, ap = level(t), level(t - 1)
        sigma = eta * math.sqrt((1 - ap) / (1 - a) * (1 - a / ap))
        k0, k1 = math.sqrt(ap), math.sqrt(1 - ap)
        if i == len(ev) - 1:
            k0, k1 = 1.0, 0.0
        u0, u1 = 1.0, 0.0
        if i + 1 < len(ev) and ev[i + 1] >= t:
            rho = level(ev[i + 1]) / ap
            u0, u1 = math.sqrt(rho), math.sqrt(1 - rho)
        rows.append([1 / math.sqrt(a), -math.sqrt(1 - a) / math.sqrt(a), -bound, bound, math.sqrt(ap),
                     math.sqrt(max(1 - ap - sigma ** 2, 0.0)), sigma, k0, k1, u0, u1, 0.0])
    return g, rows


@pytest.mark.parametrize("case", sorted(SEQUENCES))
@pytest.mark.parametrize("eta,one", [(0.0, False), (0.7, False), (0.7, True)])
def test_sequence_rows_and_draws(case, eta, one):
    from afldm_amd.schedulers.schedule import ROW_WIDTH
    n, jl, js = case
    s = sched(set_alpha_to_one=one)
    assert s.repaint_evaluations(n, jl, js) == SEQUENCES[case]
    rp = s.repaint_schedule(n, eta=eta, jump_length=jl, jump_n_sample=js)
    ev = SEQUENCES[case]
    g, want = want_rows(sched(set_alpha_to_one=one), n, ev, eta)
    assert ROW_WIDTH["repaint"] == 12 and rp.kind == "repaint" and rp.noise_dtype is None and rp.init_noise_sigma == 1.0
    assert list(rp.timesteps) == [g[n - 1 - t] for t in ev] and g == sorted(g, reverse=True)
    assert len(rp.rows) == len(rp.draws) == len(ev) and all(len(r) == 12 for r in rp.rows)
    got = rp.table("cpu")
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(ev), 12)
    assert torch.equal(got, torch.tensor(want, dtype=torch.float64).float())        # to fp32 rounding: the same fp32 numbers
    torch.testing.assert_close(torch.tensor(rp.rows, dtype=torch.float64), torch.tensor(want, dtype=torch.float64),
                               rtol=1e-12, atol=1e-15)
    for i, (row, d) in enumerate(zip(rp.rows, rp.draws)):
        p, q, lo, hi, a, b, c, k0, k1, u0, u1, pad = row
        jump = i + 1 < len(ev) and ev[i + 1] >= ev[i]
        assert (u1 != 0.0) == jump and (jump or (u0, u1) == (1.0, 0.0)) and pad == 0.0
        assert (lo, hi) == (-math.inf, math.inf)
        assert abs(u0 * u0 + u1 * u1 - 1) < 1e-12 and (i == len(ev) - 1 or abs(k0 * k0 + k1 * k1 - 1) < 1e-12)
        assert abs(a * a + b * b + c * c - 1) < 1e-12                               # the reverse step keeps the level a_prev
        assert d == (k1 != 0.0, c != 0.0, u1 != 0.0) and rp.slots(i) == tuple(j for j in range(3) if d[j])
        if eta == 0.0:
            assert c == 0.0 and not d[1]
    assert rp.rows[-1][7:9] == (1.0, 0.0) and rp.draws[-1] == (False, bool(eta) and not one, False)
    # z_k: every evaluation but the last, and but those that land on final_alpha_cumprod = 1 (nothing to add there)
    assert [d[0] for d in rp.draws] == [i < len(ev) - 1 and (ev[i] > 0 or not one) for i in range(len(ev))]
    if eta:
        assert [d[1] for d in rp.draws] == [t > 0 or not one for t in ev]           # sigma = 0 at a_prev = 1 (set_alpha_to_one)


def test_default_run_has_410_evaluations():
    s = sched()
    ev = s.repaint_evaluations(50, 10, 10)
    rp = s.repaint_schedule(50)
    assert len(ev) == len(rp.timesteps) == 410 and ev[0] == 49 and ev[-1] == 0
    assert rp.config._repaint_jump_length == 10 and rp.config._repaint_jump_n_sample == 10 and rp.config._repaint_eta == 0.0
    g = [int(t) for t in s.timesteps]
    assert list(rp.timesteps) == [g[49 - t] for t in ev]
    assert sum(r[10] != 0.0 for r in rp.rows) == 4 * 9                              # 4 jump points, each taken 9 times


def test_clip_and_other_settings():
    n, ev = 6, SEQUENCES[(6, 2, 2)]
    for kw, bound in [(dict(clip_sample=True), 1.0), (dict(clip_sample=True, clip_sample_range=2.5), 2.5),
                      (dict(clip_sample=False, clip_sample_range=2.5), math.inf)]:
        rp = sched(**kw).repaint_schedule(n, 0.3, 2, 2)
        _, want = want_rows(sched(**kw), n, ev, 0.3, bound)
        assert torch.equal(rp.table("cpu"), torch.tensor(want, dtype=torch.float64).float()), kw
    # other spacings of the scheduler's timesteps: the levels follow the timesteps themselves
    for sp in ("trailing", "linspace"):
        rp = sched(timestep_spacing=sp).repaint_schedule(n, 0.3, 2, 2)
        g, want = want_rows(sched(timestep_spacing=sp), n, ev, 0.3)
        assert list(rp.timesteps) == [g[n - 1 - t] for t in ev]
        assert torch.equal(rp.table("cpu"), torch.tensor(want, dtype=torch.float64).float()), sp
    for bad in (dict(jump_length=0), dict(jump_n_sample=0), dict(jump_length=-2)):
        with pytest.raises(ValueError):
            sched().repaint_schedule(6, **bad)
    with pytest.raises(NotImplementedError):
        sched(prediction_type="v_prediction").repaint_schedule(6)


def test_keys():
    base = dict(num_inference_steps=6, eta=0.5, jump_length=2, jump_n_sample=2)
    a = sched().repaint_schedule(**base)
    assert sched().repaint_schedule(**base) is a                                   # equal settings: the same schedule
    keys = {a.key}
    for k, v in [("num_inference_steps", 8), ("eta", 0.25), ("jump_length", 3), ("jump_n_sample", 3)]:
        other = sched().repaint_schedule(**dict(base, **{k: v}))
        assert other.key not in keys, k
        keys.add(other.key)
    assert sched(clip_sample=True).repaint_schedule(**base).key not in keys
    settings = dict(a.key[1])
    assert a.key[0] == "DDIMScheduler" and settings["_repaint_steps"] == "6" and settings["_repaint_eta"] == "0.5"
    assert settings["_repaint_jump_length"] == "2" and settings["_repaint_jump_n_sample"] == "2"


def test_sde_schedules_are_unaffected():
    from afldm_amd.schedulers import schedule
    from afldm_amd.schedulers.i2sb import I2SBScheduler
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    cfg = {k: v for k, v in FFHQ_DDIM_CONFIG.items() if k != "set_alpha_to_one"}

    def made():
        return sched().stochastic_schedule(7, 0.4), I2SBScheduler.from_config(dict(cfg, clip_sample=True)).bridge_schedule(9, False)
    before = made()
    sched().repaint_schedule(6, 0.4, 2, 2)
    schedule._MADE.clear()                                                          # made again, not looked up
    sched().repaint_schedule(6, 0.4, 2, 2)
    after = made()
    for b, a in zip(before, after):
        assert a is not b and a.key == b.key and a.draws == b.draws and a.rows == b.rows and a.kind == "sde"
        assert all(isinstance(d, bool) for d in a.draws) and not any(k.startswith("_repaint") for k, _ in a.key[1])
        assert [a.slots(k) for k in range(len(a.draws))] == [(0,) if d else () for d in a.draws]
    assert before[0].draws == (True,) * 7
    assert schedule.ROW_WIDTH["sde"] == 8 and schedule.ROW_WIDTH["ddim"] == 4 and schedule.ROW_WIDTH["dpm"] == 8
    with pytest.raises(AssertionError):                                             # only "sde" and "repaint" schedules draw
        schedule.Schedule.of(sched(), "ddim", [1], [(1.0, 0.0, 1.0, 0.0)], [True], _test_only=1)


# ------------------------------------------------------------------------------------------------ pipeline
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


def test_inpaint_latents_routes_to_a_repaint_engine_in_its_own_slot(monkeypatch):
    from afldm_amd import engine
    seen = []

    class Engine:
        def __init__(self, unet, schedule, batch, steps, use_graph):
            self.schedule = schedule
            seen.append(("init", schedule.kind, batch, steps, use_graph))

        def run(self, latents, draw=None, known=None):
            seen.append(("run", tuple(known[0].shape), tuple(known[1].shape)))
            for k in range(len(self.schedule.draws)):
                for _ in self.schedule.slots(k):
                    draw()
            return latents
    monkeypatch.setattr(engine, "DenoiseEngine", Engine)
    pipe = _pipe()
    z0, m = torch.zeros(2, 4, 8, 8), torch.ones(1, 1, 8, 8)
    g = torch.Generator().manual_seed(5)
    out = pipe.inpaint_latents(z0, m, num_inference_steps=6, eta=0.7, jump_length=2, jump_n_sample=2, generator=g)
    assert tuple(out.shape) == (2, 4, 8, 8)
    assert seen == [("init", "repaint", 2, 10, True), ("run", (2, 4, 8, 8), (1, 1, 8, 8))]
    assert "_engines" not in pipe.__dict__ and len(pipe._repaint_engines) == 1
    # the start latents, then per evaluation z_k, z_u, z_b where the schedule draws them: all from the caller's generator
    rp = sched().repaint_schedule(6, 0.7, 2, 2)
    want = torch.Generator().manual_seed(5)
    for _ in range(1 + sum(len(rp.slots(k)) for k in range(10))):
        torch.randn(2, 4, 8, 8, generator=want)
    assert torch.equal(g.get_state(), want.get_state())
    # the same settings again: the cached engine; other jump parameters: another one
    pipe.inpaint_latents(z0, m, num_inference_steps=6, eta=0.7, jump_length=2, jump_n_sample=2, latents=torch.zeros(2, 4, 8, 8))
    pipe.inpaint_latents(z0, m, num_inference_steps=6, eta=0.7, jump_length=3, jump_n_sample=2)
    assert [s[:4] for s in seen if s[0] == "init"] == [("init", "repaint", 2, 10), ("init", "repaint", 2, 9)]


def test_argument_validation(monkeypatch):
    from afldm_amd import engine
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    monkeypatch.setattr(engine, "DenoiseEngine", lambda *a, **k: pytest.fail("no engine before the arguments are checked"))
    z0, m = torch.zeros(2, 4, 8, 8), torch.ones(2, 1, 8, 8)
    pipe = _pipe()
    for bad_z, bad_m, lat in [(torch.zeros(2, 3, 8, 8), m, None), (torch.zeros(2, 4, 8, 4), m, None), (torch.zeros(4, 8, 8), m, None),
                              (z0, torch.ones(2, 4, 8, 8), None), (z0, torch.ones(3, 1, 8, 8), None), (z0, torch.ones(2, 1, 4, 4), None),
                              (z0, m, torch.zeros(1, 4, 8, 8))]:
        with pytest.raises(ValueError):
            pipe.inpaint_latents(bad_z, bad_m, num_inference_steps=4, latents=lat)
    for bad in (dict(jump_length=0), dict(jump_n_sample=0)):
        with pytest.raises(ValueError):
            pipe.inpaint_latents(z0, m, num_inference_steps=4, **bad)
    # no VAE: inpaint refuses, as _deliver does
    with pytest.raises(NotImplementedError, match="VAE"):
        pipe.inpaint(torch.zeros(2, 3, 32, 32), torch.ones(1, 1, 32, 32))
    # with one: shapes are checked before anything touches the GPU (the fake VAE cannot encode)
    vp = _pipe(vae=_FakeVae())
    for img, mask in [(torch.zeros(2, 3, 32, 16), torch.ones(1, 1, 32, 32)), (torch.zeros(2, 1, 32, 32), torch.ones(1, 1, 32, 32)),
                      (torch.zeros(2, 3, 32, 32), torch.ones(1, 1, 8, 8)), (torch.zeros(2, 3, 32, 32), torch.ones(3, 1, 32, 32)),
                      (torch.zeros(2, 3, 32, 32), torch.ones(2, 3, 32, 32))]:
        with pytest.raises(ValueError):
            vp.inpaint(img, mask)
    with pytest.raises(ValueError):
        vp.inpaint(torch.zeros(2, 3, 32, 32), torch.ones(1, 1, 32, 32), mask_mode="max")
    # DPM-Solver: refused by name from both entries
    dp = _pipe(DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG), vae=_FakeVae())
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        dp.inpaint_latents(z0, m)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        dp.inpaint(torch.zeros(2, 3, 32, 32), torch.ones(1, 1, 32, 32))


def test_ops_refuse_cpu_tensors():
    from afldm_amd import ops
    x, m = torch.zeros(1, 4, 4, 4), torch.ones(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.repaint_step(x, x.permute(0, 2, 3, 1).contiguous(), x, m, torch.zeros(1, 3, 1, 4, 4, 4), torch.zeros(12),
                         torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.repaint_step_flat(x, x, x, x, (None, None, None), (1.0, 0.0, -1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mask_pool(torch.ones(1, 1, 8, 8), 2)


def test_inpaint_script_arguments_and_mask_loading(tmp_path):
    import importlib.util
    import os
    import numpy as np
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("inpaint_ffhq", os.path.join(root, "scripts", "inpaint_ffhq.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["--input_path", "a.png", "--mask_path", "m.png", "--n_steps", "20", "--jump_length", "5",
                        "--jump_n_sample", "3", "--eta", "0.5", "--seed", "7", "--output_path", "o.png"])
    assert (a.n_steps, a.jump_length, a.jump_n_sample, a.eta, a.seed, a.output_path) == (20, 5, 3, 0.5, 7, "o.png")
    assert mod.parse_args(["--random-init"]).mask_mode == "min"
    for bad in ([], ["--input_path", "a.png"], ["--random-init", "--jump_length", "0"], ["--random-init", "--jump_n_sample", "0"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    grey = np.zeros((8, 8), dtype=np.uint8)
    grey[:, 4:] = 255
    grey[0, 0] = 200
    Image.fromarray(grey).save(tmp_path / "m.png")
    m = mod.load_mask(str(tmp_path / "m.png"), 16)
    assert tuple(m.shape) == (1, 1, 16, 16) and set(m.unique().tolist()) == {0.0, 1.0}
    assert m[0, 0, :, 8:].min() == 1 and m[0, 0, 4:, :8].max() == 0 and m[0, 0, 0, 0] == 1
    assert torch.equal(mod.load_mask(str(tmp_path / "m.png"), 16, invert=True), 1 - m)
    image, hole = mod.synthetic_inputs(3, 64)
    assert tuple(image.shape) == (1, 3, 64, 64) and image.abs().max() <= 1 and float(hole.mean()) == 0.75
