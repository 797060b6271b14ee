"""DPMSolverMultistepScheduler (DPM-Solver / DPM-Solver++, Lu et al. 2022) with diffusers' surface, config keys and
defaults: from_config, set_timesteps, timesteps, init_noise_sigma, scale_model_input, order, step.

For epsilon / v / sample prediction every update of order 1-3 is LINEAR in the latent x, the model output and the
two previous converted outputs, so a step is one coefficient row (afldm_dpm_step, include/afldm_hip.h):

    m0 = p x + q model_output          (the converted output: x0 for dpmsolver++, eps for dpmsolver)
    x_out = a x + b0 m0 + b1 m1 + b2 m2 (m1, m2: the converted outputs of the two steps before)

The rows, warm-up steps of lowered order and lower-order final steps included, are a function of the step index
alone; they are computed in float64 from the schedule and rounded once to fp32.  `step` on CUDA tensors launches
afldm_dpm_step_flat; DenoiseEngine replays afldm_dpm_step over `schedule(n)` (a Schedule of kind "dpm").
Thresholding, the stochastic SDE variants and the Karras / exponential / beta sigma schedules are not linear in this
sense (or not deterministic) and raise NotImplementedError."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import ops
from ..configs import FrozenConfig
from .schedule import Schedule

_DEFAULTS = dict(
    num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
    solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
    sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
    euler_at_final=False, use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False,
    use_lu_lambdas=False, use_flow_sigmas=False, flow_shift=1.0, final_sigmas_type="zero",
    lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0,
    rescale_betas_zero_snr=False,
)

# settings whose update is not the linear form above (or is stochastic): name -> value that is supported
_UNSUPPORTED = dict(thresholding=False, use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False,
                    use_lu_lambdas=False, use_flow_sigmas=False, variance_type=None, rescale_betas_zero_snr=False)


@dataclass
class DPMSolverMultistepSchedulerOutput:
    prev_sample: torch.Tensor


class DPMSolverMultistepScheduler:
    order = 1

    def __init__(self, **kw):
        cfg = dict(_DEFAULTS)
        # keys of other schedulers' configs (DDIM's clip_sample, set_alpha_to_one, ...) are ignored, as diffusers'
        # from_config does
        cfg.update({k: v for k, v in kw.items() if k in _DEFAULTS})
        self.config = FrozenConfig(cfg)
        for k, ok in _UNSUPPORTED.items():
            if cfg[k] != ok:
                raise NotImplementedError(f"afldm_amd.DPMSolverMultistepScheduler: {k}={cfg[k]!r} is not supported "
                                          "(only the deterministic, linear multistep update is)")
        if cfg["algorithm_type"] in ("sde-dpmsolver", "sde-dpmsolver++"):
            raise NotImplementedError(f"afldm_amd.DPMSolverMultistepScheduler: algorithm_type={cfg['algorithm_type']!r} "
                                      "(stochastic) is not supported")
        if cfg["algorithm_type"] not in ("dpmsolver", "dpmsolver++"):
            raise NotImplementedError(f"{cfg['algorithm_type']} is not implemented for {self.__class__}")
        if cfg["solver_type"] not in ("midpoint", "heun"):
            raise NotImplementedError(f"{cfg['solver_type']} is not implemented for {self.__class__}")
        if cfg["solver_order"] not in (1, 2, 3):
            raise NotImplementedError(f"solver_order={cfg['solver_order']} is not implemented for {self.__class__}")
        if cfg["prediction_type"] not in ("epsilon", "v_prediction", "sample"):
            raise ValueError(f"prediction_type given as {cfg['prediction_type']} must be one of `epsilon`, `sample`, "
                             "or `v_prediction` for the DPMSolverMultistepScheduler.")
        if cfg["final_sigmas_type"] not in ("zero", "sigma_min"):
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {cfg['final_sigmas_type']}")
        if cfg["algorithm_type"] == "dpmsolver" and cfg["final_sigmas_type"] == "zero":
            raise ValueError(f"`final_sigmas_type` {cfg['final_sigmas_type']} is not supported for `algorithm_type` "
                             f"{cfg['algorithm_type']}. Please choose `sigma_min` instead.")
        T, b0, b1 = cfg["num_train_timesteps"], cfg["beta_start"], cfg["beta_end"]
        if cfg["trained_betas"] is not None:
            self.betas = torch.tensor(cfg["trained_betas"], dtype=torch.float32)
        elif cfg["beta_schedule"] == "linear":
            self.betas = torch.linspace(b0, b1, T, dtype=torch.float32)
        elif cfg["beta_schedule"] == "scaled_linear":
            self.betas = torch.linspace(b0 ** 0.5, b1 ** 0.5, T, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{cfg['beta_schedule']} is not implemented for {self.__class__}")
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.linspace(0, T - 1, T, dtype=np.float32)[::-1].copy())
        self._timesteps_host = []
        self._rows = []
        self._reset_state()

    @classmethod
    def from_config(cls, config, **kw):
        cfg = {k: v for k, v in dict(config).items() if not k.startswith("_")}
        cfg.update(kw)
        return cls(**cfg)

    def _reset_state(self):
        self.lower_order_nums = 0
        self._step_index = None
        self._hist = None            # fp32 [2, *sample.shape]: the last two converted outputs, newest first

    @property
    def step_index(self):
        return self._step_index

    @property
    def model_outputs(self):
        """diffusers' history list (oldest first, None where the warm-up has not filled it); this implementation keeps
        the two outputs before the current one."""
        out = [None] * self.config.solver_order
        if self._hist is not None:
            for k in range(min(self.lower_order_nums, self.config.solver_order, 2)):
                out[-1 - k] = self._hist[k]
        return out

    def scale_model_input(self, sample, *args, **kwargs):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        cfg = self.config
        T = cfg.num_train_timesteps
        clipped_idx = int(torch.searchsorted(torch.flip(self.lambda_t, [0]), cfg.lambda_min_clipped))
        last_timestep = T - clipped_idx
        sp = cfg.timestep_spacing
        if sp == "linspace":
            ts = np.linspace(0, last_timestep - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif sp == "leading":
            ratio = last_timestep // (num_inference_steps + 1)
            ts = (np.arange(0, num_inference_steps + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64)
            ts += cfg.steps_offset
        elif sp == "trailing":
            ratio = T / num_inference_steps
            ts = np.arange(last_timestep, 0, -ratio).round().copy().astype(np.int64) - 1
        else:
            raise ValueError(f"{sp} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        ac = self.alphas_cumprod
        train_sigmas = (((1 - ac) / ac) ** 0.5).numpy()                     # fp32, as diffusers tabulates them
        sigmas = train_sigmas[ts].astype(np.float64)
        last = float(train_sigmas[0]) if cfg.final_sigmas_type == "sigma_min" else 0.0
        self.sigmas = np.concatenate([sigmas, [last]])
        self.num_inference_steps = len(ts)
        self._timesteps_host = [int(t) for t in ts]
        self.timesteps = torch.from_numpy(ts).to(device=device, dtype=torch.int64)
        self._rows = [self._row(i) for i in range(len(ts))]
        self._reset_state()

    # ------------------------------------------------------------------ the update as coefficient rows
    def step_order(self, i):
        """Solver order of step i: lowered while the history fills (diffusers' lower_order_nums = min(i, solver_order))
        and at the end (lower_order_final / euler_at_final / final_sigmas_type='zero')."""
        cfg, n = self.config, self.num_inference_steps
        final = i == n - 1 and (cfg.euler_at_final or (cfg.lower_order_final and n < 15) or cfg.final_sigmas_type == "zero")
        second = i == n - 2 and cfg.lower_order_final and n < 15
        warm = min(i, cfg.solver_order)
        if cfg.solver_order == 1 or warm < 1 or final:
            return 1
        if cfg.solver_order == 2 or warm < 2 or second:
            return 2
        return 3

    @staticmethod
    def _alpha_sigma(sig):
        alpha = 1.0 / math.sqrt(sig * sig + 1.0)
        return alpha, sig * alpha

    def _lam(self, j):
        alpha, sigma = self._alpha_sigma(self.sigmas[j])
        return math.log(alpha) - math.log(sigma)

    def _row(self, i):
        """(p, q, a, b0, b1, b2, 0, 0) of step i in float64."""
        cfg = self.config
        pp = cfg.algorithm_type == "dpmsolver++"
        alpha_s, sigma_s = self._alpha_sigma(self.sigmas[i])
        alpha_t, sigma_t = self._alpha_sigma(self.sigmas[i + 1])
        # converted model output m0 = p x + q model_output
        if pp:
            p, q = {"epsilon": (1 / alpha_s, -sigma_s / alpha_s), "sample": (0.0, 1.0),
                    "v_prediction": (alpha_s, -sigma_s)}[cfg.prediction_type]
        else:
            p, q = {"epsilon": (0.0, 1.0), "sample": (1 / sigma_s, -alpha_s / sigma_s),
                    "v_prediction": (sigma_s, alpha_s)}[cfg.prediction_type]
        order = self.step_order(i)
        # exp(-h), h = lambda_t - lambda_s, straight from the sigmas: 0 (h = +inf) at the final sigma = 0
        em = (sigma_t / alpha_t) / (sigma_s / alpha_s) if sigma_t > 0 else 0.0
        if pp:
            a = sigma_t / sigma_s
            c0 = alpha_t * (1.0 - em)                       # -alpha_t (e^-h - 1)
        else:
            a = alpha_t / alpha_s
            c0 = -sigma_t * (1.0 / em - 1.0)                # -sigma_t (e^h - 1)
        b = np.array([c0, 0.0, 0.0])
        if order >= 2:
            h = self._lam(i + 1) - self._lam(i)
            if pp:
                phi1 = -math.expm1(-h)                      # 1 - e^-h
                d1 = alpha_t * (1.0 - phi1 / h)             # alpha_t ((e^-h - 1) / h + 1)
                d2 = -alpha_t * ((h - phi1) / (h * h) - 0.5)
            else:
                phi1 = math.expm1(h)                        # e^h - 1
                d1 = -sigma_t * (phi1 / h - 1.0)
                d2 = -sigma_t * ((phi1 - h) / (h * h) - 0.5)
            r0 = (self._lam(i) - self._lam(i - 1)) / h
            D1_0 = np.array([1.0, -1.0, 0.0]) / r0          # (m0 - m1) / r0
            if order == 2:
                c1 = 0.5 * c0 if cfg.solver_type == "midpoint" else d1
                b += c1 * D1_0
            else:
                r1 = (self._lam(i - 1) - self._lam(i - 2)) / h
                D1_1 = np.array([0.0, 1.0, -1.0]) / r1      # (m1 - m2) / r1
                D1 = D1_0 + r0 / (r0 + r1) * (D1_0 - D1_1)
                D2 = (D1_0 - D1_1) / (r0 + r1)
                b += d1 * D1 + d2 * D2
        return (p, q, a, float(b[0]), float(b[1]), float(b[2]), 0.0, 0.0)

    def schedule(self, num_inference_steps=None):
        """The sampler of `num_inference_steps` (None: of the current timesteps, solver state untouched) as the Schedule
        DenoiseEngine replays with afldm_dpm_step."""
        if num_inference_steps is not None:
            self.set_timesteps(num_inference_steps)
        elif self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' first")
        return Schedule.of(self, "dpm", self._timesteps_host, self._rows, _dpm_steps=self.num_inference_steps)

    def coefficient_table(self, device):
        """float32 [nsteps, 8] rows (p, q, a, b0, b1, b2, 0, 0) for afldm_dpm_step, rounded once from float64."""
        return self.schedule().table(device)

    # ------------------------------------------------------------------ diffusers step API
    def index_for_timestep(self, timestep):
        cand = (self.timesteps.cpu() == int(timestep)).nonzero()
        if len(cand) == 0:
            return len(self.timesteps) - 1
        return int(cand[1 if len(cand) > 1 else 0])

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict=True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if not sample.is_cuda:
            raise RuntimeError("afldm_amd.DPMSolverMultistepScheduler.step runs on MI355X tensors only (no CPU path)")
        if self._step_index is None:
            self._step_index = self.index_for_timestep(timestep)
        x = sample.to(torch.float32).contiguous()
        e = model_output.to(torch.float32).contiguous()
        if self._hist is None or self._hist.shape[1:] != x.shape or self._hist.device != x.device:
            self._hist = torch.zeros((2,) + tuple(x.shape), dtype=torch.float32, device=x.device)
        prev = ops.dpm_step_flat(x, e, self._hist, self._rows[self._step_index]).to(sample.dtype)
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        if not return_dict:
            return (prev,)
        return DPMSolverMultistepSchedulerOutput(prev_sample=prev)

    def __len__(self):
        return self.config.num_train_timesteps
