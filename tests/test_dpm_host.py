"""DPMSolverMultistepScheduler on the host: its [nsteps, 8] coefficient rows against a float64 restatement of
DPM-Solver / DPM-Solver++ orders 1-3 written from the update formulas (Lu et al. 2022, "DPM-Solver++", in diffusers'
multistep form), convergence on an analytic Gaussian model, and the diffusers surface.  No GPU needed."""
import itertools
import math

import numpy as np
import pytest
import torch

from afldm_amd.configs import FFHQ_DDIM_CONFIG


def _sched(**kw):
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**kw)


# ------------------------------------------------------------------------------------------------ the restated solver
def ref_timesteps(T, n, spacing, offset):
    if spacing == "linspace":
        return np.linspace(0, T - 1, n + 1).round()[::-1][:-1].astype(np.int64)
    if spacing == "leading":
        return (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1].astype(np.int64) + offset
    return np.arange(T, 0, -T / n).round().astype(np.int64) - 1


def ref_sigmas(betas, ts, final):
    ac = torch.cumprod(1.0 - betas, 0)
    sig = (((1 - ac) / ac) ** 0.5).double().numpy()
    return [float(sig[t]) for t in ts] + [float(sig[0]) if final == "sigma_min" else 0.0]


class RefSolver:
    """Float64 DPM-Solver(++) multistep, statement by statement from the paper's update rules."""

    def __init__(self, sigmas, order, algo, solver_type, prediction, lower_order_final=True, euler_at_final=False,
                 final="zero"):
        self.sig, self.order, self.algo, self.st, self.pred = sigmas, order, algo, solver_type, prediction
        self.lof, self.eaf, self.final = lower_order_final, euler_at_final, final
        self.n = len(sigmas) - 1
        self.outs, self.i, self.warm = [], 0, 0

    @staticmethod
    def asl(s):
        al = 1 / math.sqrt(s * s + 1)
        sg = s * al
        return al, sg, (math.log(al) - math.log(sg)) if sg > 0 else math.inf

    def convert(self, out, x):
        al, sg, _ = self.asl(self.sig[self.i])
        if self.algo == "dpmsolver++":
            return {"epsilon": (x - sg * out) / al, "sample": out, "v_prediction": al * x - sg * out}[self.pred]
        return {"epsilon": out, "sample": (x - al * out) / sg, "v_prediction": al * out + sg * x}[self.pred]

    def step(self, out, x):
        i, n = self.i, self.n
        m = self.convert(out, x)
        self.outs = (self.outs + [m])[-3:]
        final = i == n - 1 and (self.eaf or (self.lof and n < 15) or self.final == "zero")
        second = i == n - 2 and self.lof and n < 15
        at, st, lt = self.asl(self.sig[i + 1])
        a0, s0, l0 = self.asl(self.sig[i])
        pp = self.algo == "dpmsolver++"
        h = lt - l0
        if self.order == 1 or self.warm < 1 or final:
            if pp:
                xn = (st / s0) * x - at * ((math.exp(-h) if h < math.inf else 0.0) - 1) * m
            else:
                xn = (at / a0) * x - st * (math.exp(h) - 1) * m
        elif self.order == 2 or self.warm < 2 or second:
            _, _, l1 = self.asl(self.sig[i - 1])
            m0, m1 = self.outs[-1], self.outs[-2]
            r0 = (l0 - l1) / h
            D0, D1 = m0, (m0 - m1) / r0
            if pp:
                xn = (st / s0) * x - at * (math.exp(-h) - 1) * D0
                xn = xn - 0.5 * at * (math.exp(-h) - 1) * D1 if self.st == "midpoint" else \
                    xn + at * ((math.exp(-h) - 1) / h + 1) * D1
            else:
                xn = (at / a0) * x - st * (math.exp(h) - 1) * D0
                xn = xn - 0.5 * st * (math.exp(h) - 1) * D1 if self.st == "midpoint" else \
                    xn - st * ((math.exp(h) - 1) / h - 1) * D1
        else:
            _, _, l1 = self.asl(self.sig[i - 1])
            _, _, l2 = self.asl(self.sig[i - 2])
            m0, m1, m2 = self.outs[-1], self.outs[-2], self.outs[-3]
            r0, r1 = (l0 - l1) / h, (l1 - l2) / h
            D1_0, D1_1 = (m0 - m1) / r0, (m1 - m2) / r1
            D1 = D1_0 + r0 / (r0 + r1) * (D1_0 - D1_1)
            D2 = (D1_0 - D1_1) / (r0 + r1)
            if pp:
                xn = ((st / s0) * x - at * (math.exp(-h) - 1) * m0 + at * ((math.exp(-h) - 1) / h + 1) * D1
                      - at * ((math.exp(-h) - 1 + h) / h ** 2 - 0.5) * D2)
            else:
                xn = ((at / a0) * x - st * (math.exp(h) - 1) * m0 - st * ((math.exp(h) - 1) / h - 1) * D1
                      - st * ((math.exp(h) - 1 - h) / h ** 2 - 0.5) * D2)
        self.warm = min(self.warm + 1, self.order)
        self.i += 1
        return xn


def apply_rows(rows, x, outs):
    """The kernel's linear form in float64: m0 = p x + q out; x = a x + b0 m0 + b1 h1 + b2 h2; h2, h1 = h1, m0."""
    h1 = torch.zeros_like(x)
    h2 = torch.zeros_like(x)
    xs = []
    for r, out in zip(rows.tolist(), outs):
        p, q, a, b0, b1, b2 = r[:6]
        m = p * x + q * out
        x = a * x + b0 * m + b1 * h1 + b2 * h2
        h2, h1 = h1, m
        xs.append(x)
    return xs


COMBOS = [c for c in itertools.product((1, 2, 3), ("dpmsolver++", "dpmsolver"), ("midpoint", "heun"),
                                       ("linspace", "leading", "trailing"), ("zero", "sigma_min"),
                                       ("epsilon", "v_prediction", "sample"))
          if not (c[1] == "dpmsolver" and c[4] == "zero")]


@pytest.mark.parametrize("order,algo,solver_type,spacing,final,pred", COMBOS)
def test_coefficient_table_matches_restated_solver(order, algo, solver_type, spacing, final, pred):
    cfg = dict(FFHQ_DDIM_CONFIG, solver_order=order, algorithm_type=algo, solver_type=solver_type,
               timestep_spacing=spacing, final_sigmas_type=final, prediction_type=pred)
    s = _sched(**{k: v for k, v in cfg.items() if not k.startswith("_")})
    betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float32) ** 2
    g = torch.Generator().manual_seed(order * 100 + len(pred))
    for n in (10, 20, 25):
        s.set_timesteps(n)
        ts = ref_timesteps(1000, n, spacing, 1)
        assert s._timesteps_host == [int(t) for t in ts]
        table = s.coefficient_table("cpu")
        assert table.shape == (n, 8) and table.dtype == torch.float32 and torch.isfinite(table).all()
        assert (table[:, 6:] == 0).all()
        x = torch.randn(2, 4, 6, 6, generator=g, dtype=torch.float64)
        outs = [torch.randn(2, 4, 6, 6, generator=g, dtype=torch.float64) for _ in range(n)]
        got = apply_rows(table.double(), x, outs)
        ref = RefSolver(ref_sigmas(betas, ts, final), order, algo, solver_type, pred, final=final)
        xr = x
        for i in range(n):
            xr = ref.step(outs[i], xr)
            # fp32 coefficients applied to O(1..10) data: the error is the rows' rounding, relative to the terms' size
            scale = float(x.abs().max() + max(o.abs().max() for o in outs[:i + 1])) * max(1.0, float(table[:i + 1].abs().max()))
            err = float((got[i] - xr).abs().max())
            assert err <= 2e-6 * scale * (i + 1), (n, i, err, scale)


def test_zero_final_sigma_is_the_plain_x0_step():
    s = _sched()
    s.set_timesteps(20)
    p, q, a, b0, b1, b2 = s.coefficient_table("cpu")[-1, :6].tolist()
    al, sg = s._alpha_sigma(s.sigmas[-2])
    assert a == 0 and b0 == 1 and b1 == 0 and b2 == 0          # x_out = m0 = x0 prediction
    assert p == pytest.approx(1 / al, rel=1e-6) and q == pytest.approx(-sg / al, rel=1e-6)


def test_warm_up_and_final_orders():
    s = _sched(solver_order=3)
    s.set_timesteps(20)
    assert [s.step_order(i) for i in range(20)] == [1, 2] + [3] * 17 + [1]
    s.set_timesteps(10)                                        # < 15 steps: lower_order_final lowers the last two
    assert [s.step_order(i) for i in range(10)] == [1, 2] + [3] * 6 + [2, 1]
    s = _sched(solver_order=2, final_sigmas_type="sigma_min", lower_order_final=False)
    s.set_timesteps(10)
    assert [s.step_order(i) for i in range(10)] == [1] + [2] * 9


# ------------------------------------------------------------------------------------------------ analytic convergence
MU, S = 0.7, 1.0          # unit-variance data, like the VAE's scaled latents


def gaussian_run(rows_or_coef, ts_alphas, z, kind):
    """Sample from the exact eps-prediction of x0 ~ N(MU, S^2): eps(x) = sigma (x - alpha MU) / (alpha^2 S^2 + sigma^2)."""
    ac = ts_alphas
    x = math.sqrt(ac[0] * S * S + 1 - ac[0]) * z + math.sqrt(ac[0]) * MU
    h1 = h2 = torch.zeros_like(z)
    for i, r in enumerate(rows_or_coef):
        al, sg = math.sqrt(ac[i]), math.sqrt(1 - ac[i])
        eps = sg * (x - al * MU) / (al * al * S * S + sg * sg)
        if kind == "dpm":
            p, q, a, b0, b1, b2 = r[:6]
            m = p * x + q * eps
            x, h2, h1 = a * x + b0 * m + b1 * h1 + b2 * h2, h1, m
        else:
            sa_t, sb_t, sa_p, sb_p = r
            x = sa_p * (x - sb_t * eps) / sa_t + sb_p * eps
    return x


def exact_end(z, a_end):
    return math.sqrt(a_end) * MU + math.sqrt(a_end * S * S + 1 - a_end) * z


def dpm_error(n, **kw):
    s = _sched(**kw)
    s.set_timesteps(n)
    ac = s.alphas_cumprod.double()
    a_seq = [float(ac[t]) for t in s._timesteps_host]
    sig_end = s.sigmas[-1]
    a_end = 1 / (sig_end * sig_end + 1)
    z = torch.linspace(-2.5, 2.5, 41, dtype=torch.float64)
    x = gaussian_run(torch.tensor(s._rows, dtype=torch.float64).tolist(), a_seq, z, "dpm")
    return float((x - exact_end(z, a_end)).abs().max())


@pytest.mark.parametrize("order,min_rate", [(1, 0.9), (2, 1.8), (3, 2.5)])
def test_convergence_order_on_gaussian_data(order, min_rate):
    kw = dict(solver_order=order, timestep_spacing="linspace", final_sigmas_type="sigma_min", lower_order_final=False)
    # (below ~20 steps the first step, from t = 999 at sigma ~ 15, dominates: the orders show from there on)
    errs = [dpm_error(n, **kw) for n in (20, 40, 80, 160)]
    rates = [math.log2(errs[k] / errs[k + 1]) for k in range(3)]
    print(f"order {order}: errors {errs}, observed rates {rates}")
    assert errs == sorted(errs, reverse=True)
    assert rates[-1] >= min_rate and rates[-2] >= min_rate, rates


def test_dpmpp_2m_beats_ddim_at_20_steps():
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    d = ffhq_ddim_scheduler()
    d.set_timesteps(20)
    ac = d.alphas_cumprod.double()
    a_seq = [float(ac[t]) for t in d._timesteps_host]
    z = torch.linspace(-2.5, 2.5, 41, dtype=torch.float64)
    x = gaussian_run(d.coefficient_table("cpu").double().tolist(), a_seq, z, "ddim")
    ddim_err = float((x - exact_end(z, float(d.final_alpha_cumprod))).abs().max())
    cfg = {k: v for k, v in FFHQ_DDIM_CONFIG.items() if not k.startswith("_")}
    dpm_err = dpm_error(20, **cfg)
    print(f"20 steps: DDIM error {ddim_err:.3e}, DPM++ 2M error {dpm_err:.3e}")
    assert dpm_err < 0.5 * ddim_err, (dpm_err, ddim_err)


# ------------------------------------------------------------------------------------------------ surface
def test_from_ffhq_ddim_config_gives_diffusers_defaults():
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG)
    c = s.config
    assert (c.solver_order, c.algorithm_type, c.solver_type, c.lower_order_final, c.euler_at_final,
            c.final_sigmas_type, c.prediction_type) == (2, "dpmsolver++", "midpoint", True, False, "zero", "epsilon")
    assert (c.timestep_spacing, c.steps_offset, c.beta_schedule, c.beta_start, c.beta_end) == \
        ("leading", 1, "scaled_linear", 0.0015, 0.0195)
    assert "clip_sample" not in c and "set_alpha_to_one" not in c
    assert s.order == 1 and s.init_noise_sigma == 1.0 and s.schedule(5).kind == "dpm"
    assert DPMSolverMultistepScheduler().config.timestep_spacing == "linspace"
    s.set_timesteps(20)
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == [47 * k + 1 for k in range(20, 0, -1)]
    x = torch.ones(1)
    assert s.scale_model_input(x, s.timesteps[0]) is x
    with pytest.raises(RuntimeError, match="MI355X"):
        s.step(torch.zeros(1, 4, 2, 2), s.timesteps[0], torch.zeros(1, 4, 2, 2))
    # round trip through its own config
    assert dict(DPMSolverMultistepScheduler.from_config(s.config).config) == dict(c)


@pytest.mark.parametrize("kw,name", [
    (dict(thresholding=True), "thresholding"), (dict(algorithm_type="sde-dpmsolver++"), "sde-dpmsolver"),
    (dict(algorithm_type="sde-dpmsolver"), "sde-dpmsolver"), (dict(use_karras_sigmas=True), "use_karras_sigmas"),
    (dict(use_exponential_sigmas=True), "use_exponential_sigmas"), (dict(use_beta_sigmas=True), "use_beta_sigmas"),
    (dict(variance_type="learned_range"), "variance_type")])
def test_unsupported_settings_raise(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        _sched(**kw)


def test_diffusers_shim_and_alias_export_the_class():
    import sys
    from afldm_amd import compat
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    saved = {k: v for k, v in sys.modules.items() if k == "diffusers" or k.startswith("diffusers.")}
    try:
        compat.install_diffusers_shim(force=True)
        import diffusers
        from diffusers.schedulers.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler as D3
        assert diffusers.DPMSolverMultistepScheduler is DPMSolverMultistepScheduler
        assert diffusers.schedulers.DPMSolverMultistepScheduler is DPMSolverMultistepScheduler
        assert D3 is DPMSolverMultistepScheduler
    finally:
        for k in [k for k in sys.modules if k == "diffusers" or k.startswith("diffusers.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    import afldm  # noqa: F401
    from afldm.schedulers.dpmsolver import DPMSolverMultistepScheduler as A
    assert A is DPMSolverMultistepScheduler


class _FakeUnet:
    dtype, device = torch.float32, torch.device("cpu")

    class config:
        in_channels, sample_size = 4, 8


def test_pipeline_keeps_ddim_and_the_harness_rejects_dpm(monkeypatch):
    from afldm_amd import engine, harness
    from afldm_amd.pipelines import ldm_pipeline
    from afldm_amd.schedulers.ddim import DDIMScheduler, ffhq_ddim_scheduler
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    seen = []

    class Engine:
        def __init__(self, unet, sched, batch, steps, use_graph):
            seen.append((sched.key[0], sched.kind, use_graph))
            self.scheduler = sched

        def run(self, latents):
            return latents
    monkeypatch.setattr(engine, "DenoiseEngine", Engine)
    pipe = ldm_pipeline.MyLDMPipeline(None, _FakeUnet(), ffhq_ddim_scheduler())
    pipe(latents=torch.zeros(1, 4, 8, 8), num_inference_steps=5, output_type="latent")
    assert type(pipe.scheduler) is DDIMScheduler and seen[-1] == ("DDIMScheduler", "ddim", True)
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, solver_order=3)
    pipe(latents=torch.zeros(1, 4, 8, 8), num_inference_steps=5, output_type="latent", eta=0.5, use_graph=False)
    assert type(pipe.scheduler) is DPMSolverMultistepScheduler and pipe.scheduler.config.solver_order == 3
    assert seen[-1] == ("DPMSolverMultistepScheduler", "dpm", False)
    # same config keys, other class: the engine cache must not hand the DDIM engine back
    assert len({k[5] for k in [next(iter(pipe._engines))]}) == 1 and next(iter(pipe._engines))[5] == "DPMSolverMultistepScheduler"
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        harness.shift_ldm(pipe, num_inference_steps=5)
    with pytest.raises(NotImplementedError, match="DPM"):
        pipe.ddim_inversion(torch.zeros(1, 4, 8, 8))
