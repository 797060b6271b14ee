"""DDIMScheduler with the diffusers surface the reference uses (ldm_pipeline.py:80-109,
scripts/shift_ldm_ffhq.py:85-106): from_config, set_timesteps, timesteps, scale_model_input,
step, alphas_cumprod, final_alpha_cumprod, init_noise_sigma, config.

The schedule tables are a few hundred host floats; `step` on CUDA tensors launches the HIP
update kernel (afldm_ddim_step_flat).  eta = 0 / epsilon prediction / no clipping — the
reference's configuration (configs/ldm/noise_scheduler.json:1-14); other settings raise.  `stochastic_schedule`
tabulates the eta != 0 update for the graph-replayed engine (afldm_sde_step)."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import ops
from ..utils import randn_tensor
from ..configs import FFHQ_DDIM_CONFIG, FrozenConfig
from .schedule import Schedule


def hires_kappa(t, num_train_timesteps, scale):
    """DemoFusion's cosine factor of timestep t, (1 + cos(pi (T - t) / T)) / 2 - 1 at the noisiest end of the training schedule,
    0 at t = 0 - to the power `scale`; 0 for a scale of None (the term is switched off).  hires_schedule's r, g and f."""
    T = int(num_train_timesteps)
    return 0.0 if scale is None else (0.5 * (1.0 + math.cos(math.pi * (T - int(t)) / T))) ** float(scale)


@dataclass
class DDIMSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class DDIMScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                 prediction_type="epsilon", timestep_spacing="leading", **extra):
        cfg = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                   beta_schedule=beta_schedule, trained_betas=trained_betas, clip_sample=clip_sample,
                   set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset, prediction_type=prediction_type,
                   timestep_spacing=timestep_spacing)
        cfg.update(extra)
        self.config = FrozenConfig(cfg)
        if trained_betas is not None:
            self.betas = torch.tensor(trained_betas, dtype=torch.float32)
        elif beta_schedule == "linear":
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps,
                                        dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented for {self.__class__}")
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    @classmethod
    def from_config(cls, config, **kw):
        cfg = {k: v for k, v in dict(config).items() if not k.startswith("_")}
        cfg.update(kw)
        return cls(**cfg)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError(f"num_inference_steps {num_inference_steps} > num_train_timesteps {T}")
        self.num_inference_steps = num_inference_steps
        sp = self.config.timestep_spacing
        if sp == "leading":
            ratio = T // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
            ts += self.config.steps_offset
        elif sp == "trailing":
            ratio = T / num_inference_steps
            ts = np.round(np.arange(T, 0, -ratio)).astype(np.int64) - 1
        elif sp == "linspace":
            ts = np.linspace(0, T - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        else:
            raise ValueError(sp)
        self._timesteps_host = [int(t) for t in ts]
        self.timesteps = torch.from_numpy(ts).to(device)

    def coefficients(self, timestep):
        """(sqrt a_t, sqrt(1-a_t), sqrt a_prev, sqrt(1-a_prev)) in fp32 arithmetic, as floats."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        return (float(a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_prev ** 0.5), float((1 - a_prev) ** 0.5))

    def _variance(self, timestep):
        """diffusers DDIMScheduler._get_variance: (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev), as a float."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        return float((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))

    def schedule(self, num_inference_steps):
        """The eta = 0 sampler of `num_inference_steps` as the Schedule DenoiseEngine replays with afldm_ddim_step."""
        self.set_timesteps(num_inference_steps)
        return Schedule.of(self, "ddim", self._timesteps_host, self.coefficients, _ddim_steps=int(num_inference_steps))

    def coefficient_table(self, device):
        """float32 [nsteps, 4] device table of the current timesteps (afldm_ddim_step)."""
        return self.schedule(self.num_inference_steps).table(device)

    def sde_coefficients(self, timestep, eta):
        """(p, q, lo, hi, a, b, d, c) of the stochastic step (diffusers DDIMScheduler.step with eta, epsilon prediction, no clip)
        in float64 from the fp32 alphas_cumprod, for afldm_sde_step: x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t) unclipped,
        x_prev = sqrt(a_prev) x0 + sqrt(max(1 - a_prev - sigma^2, 0)) eps + sigma z, sigma = eta sqrt(_variance(t))."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        sigma = float(eta) * math.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))
        return (1 / math.sqrt(a_t), -math.sqrt(1 - a_t) / math.sqrt(a_t), -math.inf, math.inf,
                0.0, math.sqrt(a_prev), math.sqrt(max(1 - a_prev - sigma * sigma, 0.0)), sigma)

    def stochastic_schedule(self, num_inference_steps, eta):
        """The eta != 0 sampler of `num_inference_steps` as the Schedule DenoiseEngine replays with afldm_sde_step.  Every step
        draws, the last one included (its sigma is 0 with set_alpha_to_one, but step() still draws): randn_tensor in the
        model's dtype, as step() draws with the model output's."""
        if self.config.clip_sample or self.config.prediction_type != "epsilon":
            raise NotImplementedError("afldm_amd.DDIMScheduler implements the reference's setting: "
                                      "epsilon prediction, clip_sample=False")
        self.set_timesteps(num_inference_steps)
        ts = self._timesteps_host
        return Schedule.of(self, "sde", ts, lambda t: self.sde_coefficients(t, eta), [True] * len(ts),
                           _ddim_steps=int(num_inference_steps), _ddim_eta=float(eta))

    def seeded_schedule(self, num_inference_steps, eta):
        """stochastic_schedule(num_inference_steps, eta) for the seeded samplers (SeededEngine, SeededSlotEngine): the same rows,
        float for float, as kind "seeded" - afldm_seeded_step makes every step's noise in registers from the sample's seed and
        the step's ordinal, so nothing is drawn - under a key of its own."""
        sde = self.stochastic_schedule(num_inference_steps, eta)
        return Schedule.of(self, "seeded", sde.timesteps, sde.rows, _seeded_steps=int(num_inference_steps), _seeded_eta=float(eta))

    def panorama_schedule(self, num_inference_steps, eta=0.0):
        """MultiDiffusion sampling of a canvas larger than the model's window (Bar-Tal et al., ICML 2023) over this scheduler's
        `num_inference_steps` timesteps, as the Schedule PanoramaEngine replays with afldm_pano_step: the rows are
        sde_coefficients(t, eta), applied per window and averaged over the windows that cover a canvas element.  Unlike
        stochastic_schedule a step draws - one randn_tensor of the CANVAS's shape in the model's dtype - only where its sigma is
        not 0: eta = 0 draws nothing, and with set_alpha_to_one neither does the last step."""
        if self.config.clip_sample or self.config.prediction_type != "epsilon":
            raise NotImplementedError("afldm_amd.DDIMScheduler implements the reference's setting: "
                                      "epsilon prediction, clip_sample=False")
        self.set_timesteps(num_inference_steps)
        ts = self._timesteps_host
        rows = [self.sde_coefficients(t, eta) for t in ts]
        return Schedule.of(self, "pano", ts, rows, [r[7] != 0.0 for r in rows], _pano_steps=int(num_inference_steps),
                           _pano_eta=float(eta))

    def pag_schedule(self, num_inference_steps, eta=0.0, pag_scale=3.0, guidance_rescale=0.0):
        """Perturbed-attention guidance (Ahn et al. 2024; diffusers PAGMixin) over this scheduler's `num_inference_steps`
        timesteps, as the Schedule PAGEngine replays with afldm_pag_step: every evaluation runs the UNet and the perturbed UNet
        as one batch, forms g = e + pag_scale (e - e_p), rescales it per sample towards std(e) by `guidance_rescale` (diffusers
        rescale_noise_cfg) and applies the row of stochastic_schedule(num_inference_steps, eta) to g.  The first eight fields
        of a row are that schedule's, float for float; then pag_scale, guidance_rescale, 0, 0.  With eta != 0 the draws are
        stochastic_schedule's too (every step, in the model's dtype); eta = 0 has c = 0 in every row and draws nothing, like the
        plain eta = 0 sampler."""
        s, phi = float(pag_scale), float(guidance_rescale)
        if s < 0.0 or not 0.0 <= phi <= 1.0:
            raise ValueError(f"pag_schedule: pag_scale = {pag_scale} must be >= 0 and guidance_rescale = {guidance_rescale} in [0, 1]")
        sde = self.stochastic_schedule(num_inference_steps, eta)
        rows = [r + (s, phi, 0.0, 0.0) for r in sde.rows]
        draws = sde.draws if float(eta) != 0.0 else [False] * len(rows)
        return Schedule.of(self, "pag", sde.timesteps, rows, draws, _pag_steps=int(num_inference_steps), _pag_eta=float(eta),
                           _pag_scale=s, _pag_rescale=phi)

    def cfg_schedule(self, num_inference_steps, eta=0.0, guidance_scale=3.0, guidance_rescale=0.0):
        """Classifier-free guidance (Ho & Salimans 2022) over class labels on this scheduler's `num_inference_steps` timesteps, as
        the Schedule CFGEngine replays with afldm_pag_step: every evaluation runs the UNet on the conditional and the
        unconditional rows as one batch, e_c and e_u, forms g = e_c + (guidance_scale - 1) (e_c - e_u) - diffusers'
        e_u + guidance_scale (e_c - e_u) in another order of operations - rescales it per sample towards std(e_c) by
        `guidance_rescale` (diffusers rescale_noise_cfg) and applies the row of stochastic_schedule(num_inference_steps, eta)
        to g.  The first eight fields of a row are that schedule's, float for float; then guidance_scale - 1,
        guidance_rescale, 0, 0.  The draws are as in pag_schedule.  guidance_scale = 1 is the conditional sampler."""
        w, phi = float(guidance_scale), float(guidance_rescale)
        if not w >= 1.0 or not 0.0 <= phi <= 1.0:
            raise ValueError(f"cfg_schedule: guidance_scale = {guidance_scale} must be >= 1 and guidance_rescale = "
                             f"{guidance_rescale} in [0, 1]")
        sde = self.stochastic_schedule(num_inference_steps, eta)
        rows = [r + (w - 1.0, phi, 0.0, 0.0) for r in sde.rows]
        draws = sde.draws if float(eta) != 0.0 else [False] * len(rows)
        return Schedule.of(self, "cfg", sde.timesteps, rows, draws, _cfg_steps=int(num_inference_steps), _cfg_eta=float(eta),
                           _cfg_scale=w, _cfg_rescale=phi)

    def sag_schedule(self, num_inference_steps, eta=0.0, sag_scale=0.75, guidance_rescale=0.0):
        """Self-attention guidance (Hong et al., ICCV 2023; diffusers StableDiffusionSAGPipeline) over this scheduler's
        `num_inference_steps` timesteps, as the Schedule SAGEngine replays: every step evaluates the UNet, degrades its input where
        one site's attention mass exceeds 1 (afldm_sag_degrade, which reads p and q of the row), evaluates the UNet again and
        applies afldm_pag_step with the second output in the perturbed one's place, g = e + sag_scale (e - e_d).  Rows and draws
        are pag_schedule(num_inference_steps, eta, sag_scale, guidance_rescale)'s, float for float; the kind is "sag", so that
        an engine of one kind never replays the other's schedule."""
        s, phi = float(sag_scale), float(guidance_rescale)
        if s < 0.0 or not 0.0 <= phi <= 1.0:
            raise ValueError(f"sag_schedule: sag_scale = {sag_scale} must be >= 0 and guidance_rescale = {guidance_rescale} in [0, 1]")
        pag = self.pag_schedule(num_inference_steps, eta, s, phi)
        return Schedule.of(self, "sag", pag.timesteps, pag.rows, pag.draws, _sag_steps=int(num_inference_steps),
                           _sag_eta=float(eta), _sag_scale=s, _sag_rescale=phi)

    def _reverse_row(self, ab, ab_prev, eta):
        """(p, q, lo, hi, a, b, c) of one reverse step from level ab to ab_prev (epsilon prediction), the first seven fields of
        a "repaint" or "ilvr" row: x0 = clamp((x - sqrt(1-ab) eps) / sqrt(ab), -r, r) with r = clip_sample_range under
        clip_sample and inf without; x' = sqrt(ab_prev) x0 + sqrt(1 - ab_prev - sigma^2) eps + sigma z, sigma = eta
        sqrt(DDIM's _get_variance)."""
        bound = math.inf
        if self.config.clip_sample:
            bound = float(self.config["clip_sample_range"]) if "clip_sample_range" in self.config else 1.0
        sigma = float(eta) * math.sqrt((1 - ab_prev) / (1 - ab) * (1 - ab / ab_prev))
        return (1 / math.sqrt(ab), -math.sqrt(1 - ab) / math.sqrt(ab), -bound, bound, math.sqrt(ab_prev),
                math.sqrt(max(1 - ab_prev - sigma * sigma, 0.0)), sigma)

    @staticmethod
    def repaint_evaluations(num_inference_steps, jump_length, jump_n_sample):
        """The indices t (N - 1 = the noisiest of the scheduler's timesteps ... 0 = the last) of RePaint's UNet evaluations:
        diffusers RePaintScheduler.set_timesteps walks down the schedule and, at every multiple of jump_length below
        N - jump_length, goes back up jump_length indices jump_n_sample - 1 times; the downward moves are the evaluations."""
        n, jl, js = int(num_inference_steps), int(jump_length), int(jump_n_sample)
        jumps = {j: js - 1 for j in range(0, n - jl, jl)}
        t, seq = n, []
        while t >= 1:
            t -= 1
            seq.append(t)
            if jumps.get(t, 0) > 0:
                jumps[t] -= 1
                for _ in range(jl):
                    t += 1
                    seq.append(t)
        return [t for i, t in enumerate(seq) if i == 0 or t < seq[i - 1]]

    def repaint_schedule(self, num_inference_steps, eta=0.0, jump_length=10, jump_n_sample=10):
        """RePaint inpainting (Lugmayr et al., CVPR 2022, Algorithm 1; diffusers RePaintPipeline / RePaintScheduler) over this
        scheduler's `num_inference_steps` timesteps g[0] > ... > g[N-1], as the Schedule DenoiseEngine replays with
        afldm_repaint_step.  Index t stands for g[N-1-t]; level(t) = alphas_cumprod[g[N-1-t]], level(-1) =
        final_alpha_cumprod.  For evaluation t, with ab = level(t), ab' = level(t-1) and sigma = eta sqrt(DDIM's _get_variance):
          x0 = clamp((x - sqrt(1-ab) eps) / sqrt(ab));  unknown = sqrt(ab') x0 + sqrt(1 - ab' - sigma^2) eps + sigma z_u
          known' = sqrt(ab') known + sqrt(1-ab') z_k;   y = m known' + (1 - m) unknown
        and the last evaluation takes known' = known, so that kept latents are returned exactly.  Where the next evaluation t'
        is not lower (t' >= t) the sample is noised back up to level(t'): x_out = sqrt(rho) y + sqrt(1 - rho) z_b with rho =
        level(t') / level(t-1).  That ONE Gaussian step has the same distribution as diffusers' jump_length single-beta
        `undo_step`s, with one draw where diffusers makes jump_length * stride of them: the sample follows RePaint's law, not
        diffusers' random stream.  Draws per evaluation, in this order and each only where its coefficient is not 0: z_k, z_u,
        z_b - one randn_tensor of the latent shape in the model's dtype each."""
        n, jl, js = int(num_inference_steps), int(jump_length), int(jump_n_sample)
        if jl < 1 or js < 1:
            raise ValueError(f"repaint_schedule: jump_length = {jump_length} and jump_n_sample = {jump_n_sample} must be >= 1")
        if self.config.prediction_type != "epsilon":
            raise NotImplementedError("afldm_amd.DDIMScheduler.repaint_schedule implements epsilon prediction")
        self.set_timesteps(n)
        g = self._timesteps_host

        def level(t):
            return float(self.alphas_cumprod[g[n - 1 - t]]) if t >= 0 else float(self.final_alpha_cumprod)
        ev = self.repaint_evaluations(n, jl, js)
        rows, draws = [], []
        for i, t in enumerate(ev):
            ab, ab_prev = level(t), level(t - 1)
            reverse = self._reverse_row(ab, ab_prev, eta)
            sigma = reverse[6]
            last = i == len(ev) - 1
            k0, k1 = (1.0, 0.0) if last else (math.sqrt(ab_prev), math.sqrt(1 - ab_prev))
            u0, u1 = 1.0, 0.0
            if not last and ev[i + 1] >= t:
                rho = level(ev[i + 1]) / ab_prev
                u0, u1 = math.sqrt(rho), math.sqrt(1 - rho)
            rows.append(reverse + (k0, k1, u0, u1, 0.0))
            draws.append((k1 != 0.0, sigma != 0.0, u1 != 0.0))
        return Schedule.of(self, "repaint", [g[n - 1 - t] for t in ev], rows, draws, _repaint_steps=n, _repaint_eta=float(eta),
                           _repaint_jump_length=jl, _repaint_jump_n_sample=js)

    def outpaint_schedule(self, num_inference_steps, eta=0.0, jump_length=10, jump_n_sample=10):
        """Outpainting: RePaint on a MultiDiffusion canvas larger than the model's window, as the Schedule OutpaintEngine replays
        with afldm_pano_repaint_step.  Timesteps, rows and draws are repaint_schedule(num_inference_steps, eta, jump_length,
        jump_n_sample)'s, float for float (and it refuses what that refuses); a draw is one randn_tensor of the CANVAS's shape.
        The kind is "outpaint" and the settings are its own, so that an engine of one kind never replays the other's schedule."""
        rp = self.repaint_schedule(num_inference_steps, eta, jump_length, jump_n_sample)
        return Schedule.of(self, "outpaint", rp.timesteps, rp.rows, rp.draws, _outpaint_steps=int(num_inference_steps),
                           _outpaint_eta=float(eta), _outpaint_jump_length=int(jump_length),
                           _outpaint_jump_n_sample=int(jump_n_sample))

    def _hires_kappa(self, t, scale):
        return hires_kappa(t, self.config.num_train_timesteps, scale)

    def hires_schedule(self, num_inference_steps, eta=0.0, cosine_scale_1=3.0, cosine_scale_2=1.0, cosine_scale_3=1.0):
        """High-resolution sampling on a canvas of scale x the model's window (after DemoFusion, Du et al., CVPR 2024) over this
        scheduler's `num_inference_steps` timesteps g[0] > ... > g[N-1], as the Schedule HiresEngine replays with
        afldm_hires_step.  For evaluation i, with ab = alphas_cumprod[g[i]], ab' the next level (final_alpha_cumprod after the
        last) and kappa(t) = (1 + cos(pi (T - t) / T)) / 2, T = num_train_timesteps, the row is
          (p, q, lo, hi, a, b, c) = _reverse_row(ab, ab', eta)      the reverse step, applied to the mixed predictions
          g = kappa(g[i]) ^ cosine_scale_2                          the weight of the dilated window's prediction against the local mean
          k0, k1 = sqrt(ab'), sqrt(1 - ab')                         the upsampled reference noised to the next level ...
          r = kappa(g[i+1]) ^ cosine_scale_1                        ... and the skip residual towards it
          f = kappa(g[i+1]) ^ cosine_scale_3                        how far the NEXT evaluation's dilated views are low-passed
        and the last evaluation has k0 = 1, k1 = 0, r = 0, f = 0: it returns the reverse step itself.  A cosine scale of None
        switches its term off in every row (r = 0, g = 0 or f = 0).  A step draws - one randn_tensor of the CANVAS's shape in
        the model's dtype - only where c is not 0.  hires_start gives the first evaluation's level and low-pass."""
        if self.config.clip_sample or self.config.prediction_type != "epsilon":
            raise NotImplementedError("afldm_amd.DDIMScheduler implements the reference's setting: "
                                      "epsilon prediction, clip_sample=False")
        n = int(num_inference_steps)
        self.set_timesteps(n)
        ts = self._timesteps_host
        power = self._hires_kappa
        rows = []
        for i, t in enumerate(ts):
            last = i == n - 1
            ab = float(self.alphas_cumprod[t])
            ab_prev = float(self.final_alpha_cumprod) if last else float(self.alphas_cumprod[ts[i + 1]])
            tail = (1.0, 0.0, 0.0, power(t, cosine_scale_2), 0.0) if last else (
                math.sqrt(ab_prev), math.sqrt(1 - ab_prev), power(ts[i + 1], cosine_scale_1), power(t, cosine_scale_2),
                power(ts[i + 1], cosine_scale_3))
            rows.append(self._reverse_row(ab, ab_prev, eta) + tail)
        unit = {k: None if v is None else float(v) for k, v in (("_hires_cosine_scale_1", cosine_scale_1),
                                                                ("_hires_cosine_scale_2", cosine_scale_2),
                                                                ("_hires_cosine_scale_3", cosine_scale_3))}
        return Schedule.of(self, "hires", ts, rows, [r[6] != 0.0 for r in rows], _hires_steps=n, _hires_eta=float(eta), **unit)

    def hires_start(self, num_inference_steps, cosine_scale_3=1.0):
        """(sqrt(ab_0), sqrt(1 - ab_0), f_0) of hires_schedule's first evaluation: the canvas starts as sqrt(ab_0) ref +
        sqrt(1 - ab_0) eps_ref, and the first UNet input's dilated views are low-passed by f_0 = kappa(g[0]) ^ cosine_scale_3 (0
        for None)."""
        self.set_timesteps(int(num_inference_steps))
        t0 = self._timesteps_host[0]
        ab = float(self.alphas_cumprod[t0])
        return math.sqrt(ab), math.sqrt(1 - ab), self._hires_kappa(t0, cosine_scale_3)

    def _sdedit_timesteps(self, num_inference_steps, strength):
        """The reference's get_timesteps (video_equiv_editing_pipeline.py:320-328): the last min(int(N strength), N) of the N
        timesteps.  Raises ValueError for a strength outside [0, 1] or one that leaves no evaluation."""
        n_all, strength = int(num_inference_steps), float(strength)
        if not 0.0 <= strength <= 1.0:
            raise ValueError(f"sdedit_schedule: strength = {strength} must be in [0, 1]")
        init = min(int(n_all * strength), n_all)
        t_start = max(n_all - init, 0)
        self.set_timesteps(n_all)
        ts = self._timesteps_host[t_start:]
        if not ts:
            raise ValueError(f"sdedit_schedule: strength = {strength} leaves none of the {n_all} steps (int({n_all} * {strength}) = 0)")
        return ts

    def sdedit_schedule(self, num_inference_steps, strength, eta=0.0):
        """Image-to-image sampling: SDEdit (Meng et al., ICLR 2022) with a per-element change map (Differential Diffusion, Levin &
        Fried 2023), as the Schedule SDEditEngine replays with afldm_sdedit_step.  The timesteps are the reference's
        get_timesteps: the last n = min(int(N strength), N) of this scheduler's N = `num_inference_steps`, g[0] > ... > g[n-1].
        For evaluation k, with ab = alphas_cumprod[g[k]] and ab' the next level (final_alpha_cumprod after the last):
          (p, q, lo, hi, a, b, c) = _reverse_row(ab, ab', eta)      the reverse step of a released element
          k0, k1 = sqrt(ab'), sqrt(1 - ab')                         the original noised to the next level with the run's ONE noise z
          thr = (n - 1 - k) / n                                     an element of change value <= thr is held on that trajectory
        and the last evaluation has k0 = 1, k1 = 0 and thr = 0: what is still held then (change value <= 0) is the original
        exactly, and a change value of 1 is never held (thr_0 = 1 - 1 / n).  A step draws z_u - one randn_tensor of the latent
        shape in the model's dtype - only where c is not 0.  sdedit_start gives the level the run starts from."""
        if self.config.prediction_type != "epsilon":
            raise NotImplementedError("afldm_amd.DDIMScheduler.sdedit_schedule implements epsilon prediction")
        ts = self._sdedit_timesteps(num_inference_steps, strength)
        n = len(ts)
        rows = []
        for k, t in enumerate(ts):
            last = k == n - 1
            ab = float(self.alphas_cumprod[t])
            ab_prev = float(self.final_alpha_cumprod) if last else float(self.alphas_cumprod[ts[k + 1]])
            k0, k1 = (1.0, 0.0) if last else (math.sqrt(ab_prev), math.sqrt(1 - ab_prev))
            rows.append(self._reverse_row(ab, ab_prev, eta) + (k0, k1, (n - 1 - k) / n, 0.0, 0.0))
        return Schedule.of(self, "sdedit", ts, rows, [r[6] != 0.0 for r in rows], _sdedit_steps=int(num_inference_steps),
                           _sdedit_strength=n, _sdedit_eta=float(eta))

    def sdedit_start(self, num_inference_steps, strength):
        """(k0_start, k1_start) = (sqrt(ab_0), sqrt(1 - ab_0)) of sdedit_schedule's first timestep: the run starts from
        k0_start orig + k1_start z (the reference's add_noise at the truncated schedule's first timestep)."""
        ab = float(self.alphas_cumprod[self._sdedit_timesteps(num_inference_steps, strength)[0]])
        return math.sqrt(ab), math.sqrt(1 - ab)

    def seeded_sdedit_schedule(self, num_inference_steps, strength, eta=0.0):
        """sdedit_schedule(num_inference_steps, strength, eta) for the slot sampler (EditSlotEngine): the same timesteps and rows,
        float for float, as kind "seeded_sdedit" - afldm_slot_step_edit makes z_u and the run's fixed noise z in registers from
        the request's seed, so nothing is drawn - under a key of its own.  sdedit_start gives the level the run starts from."""
        sd = self.sdedit_schedule(num_inference_steps, strength, eta)
        return Schedule.of(self, "seeded_sdedit", sd.timesteps, sd.rows, _seeded_sdedit_steps=int(num_inference_steps),
                           _seeded_sdedit_evaluations=len(sd.rows), _seeded_sdedit_eta=float(eta))

    def seeded_repaint_schedule(self, num_inference_steps, eta=0.0, jump_length=10, jump_n_sample=10):
        """repaint_schedule(num_inference_steps, eta, jump_length, jump_n_sample) for the slot sampler (EditSlotEngine): the same
        timesteps and rows, float for float, as kind "seeded_repaint" - afldm_slot_step_edit makes z_k, z_u and z_b in registers
        from the request's seed and the evaluation's ordinal, so nothing is drawn - under a key of its own."""
        rp = self.repaint_schedule(num_inference_steps, eta, jump_length, jump_n_sample)
        return Schedule.of(self, "seeded_repaint", rp.timesteps, rp.rows, _seeded_repaint_steps=int(num_inference_steps),
                           _seeded_repaint_eta=float(eta), _seeded_repaint_jump_length=int(jump_length),
                           _seeded_repaint_jump_n_sample=int(jump_n_sample))

    def reversible_levels(self, num_inference_steps, strength=None):
        """(tau, ab) of the bit-reversible sampler: tau[1] < ... < tau[N] this scheduler's timesteps in ascending order (with
        `strength`, those of _sdedit_timesteps), tau[0] = None, and ab[0] = final_alpha_cumprod, ab[k] = alphas_cumprod[tau[k]],
        as Python floats."""
        if strength is None:
            self.set_timesteps(int(num_inference_steps))
            ts = self._timesteps_host
        else:
            ts = self._sdedit_timesteps(num_inference_steps, strength)
        tau = [None] + sorted(int(t) for t in ts)
        return tau, [float(self.final_alpha_cumprod)] + [float(self.alphas_cumprod[t]) for t in tau[1:]]

    @staticmethod
    def ddim_map(ab, k, j):
        """(A, B) of the deterministic DDIM map from level k to level j given eps, x_j = A x_k + B eps, in float64:
        A = sqrt(ab_j / ab_k), B = sqrt(1 - ab_j) - A sqrt(1 - ab_k)."""
        A = math.sqrt(ab[j] / ab[k])
        return A, math.sqrt(1 - ab[j]) - A * math.sqrt(1 - ab[k])

    def reversible_schedule(self, num_inference_steps, direction, from_code, strength=None, eta=None):
        """The bit-reversible sampler - a two-step (leapfrog) form of DDIM, after BDIA (Zhang et al., ECCV 2024) at gamma = 1 - as
        the Schedule ReversibleEngine replays with afldm_rev_step on a pair (far, near) of int64 latents.  Levels as
        reversible_levels; (A, B)(k -> j) as ddim_map.  The interior row of level k is
          cx_k = A(k -> k-1) - A(k -> k+1),  ce_k = B(k -> k-1) - B(k -> k+1)       X_{k-1} = X_{k+1} + Q_k(X_k)
        formed in float64 and rounded once to fp32 by Schedule.table.  Rows (timestep; cx, ce, sign, boot):
          direction "sample", from noise X_N:         (tau_N; A(N -> N-1) - 1, B(N -> N-1), +1, 1), then k = N-1 .. 1: (tau_k; cx_k, ce_k, +1, 0)
          direction "sample", from_code (X_N, X_N-1): the interior rows only, N - 1 evaluations
          direction "invert", from an image X_0:      (tau_1; A(0 -> 1) - 1, B(0 -> 1), +1, 1), then k = 1 .. N-1: (tau_k; cx_k, ce_k, -1, 0)
          direction "invert", from_code (X_1, X_0):   the interior rows only
        The evaluation at level 0 uses tau_1, as the reference's inversion does.  Sampling ends with near = X_0, far = X_1;
        inverting with near = X_N, far = X_N-1.  Only the deterministic epsilon-prediction sampler without clipping has this
        form: anything else raises NotImplementedError."""
        if self.config.clip_sample or self.config.prediction_type != "epsilon":
            raise NotImplementedError("afldm_amd.DDIMScheduler.reversible_schedule implements the reference's setting: "
                                      "epsilon prediction, clip_sample=False")
        if eta is not None and float(eta) != 0.0:
            raise NotImplementedError("afldm_amd.DDIMScheduler.reversible_schedule: eta != 0 adds noise, which the inverse cannot "
                                      "take away again")
        if direction not in ("sample", "invert"):
            raise ValueError(f"reversible_schedule: direction {direction!r} (want 'sample' or 'invert')")
        tau, ab = self.reversible_levels(num_inference_steps, strength)
        N = len(tau) - 1
        if from_code and N < 2:
            raise ValueError(f"reversible_schedule: a code holds two levels, and this schedule has {N}")

        def interior(k, sign):
            (Ad, Bd), (Au, Bu) = self.ddim_map(ab, k, k - 1), self.ddim_map(ab, k, k + 1)
            return tau[k], (Ad - Au, Bd - Bu, float(sign), 0.0)

        if direction == "sample":
            A, B = self.ddim_map(ab, N, N - 1)
            rows = [(tau[N], (A - 1.0, B, 1.0, 1.0))] + [interior(k, +1) for k in range(N - 1, 0, -1)]
        else:
            A, B = self.ddim_map(ab, 0, 1)
            rows = [(tau[1], (A - 1.0, B, 1.0, 1.0))] + [interior(k, -1) for k in range(1, N)]
        if from_code:
            rows = rows[1:]
        return Schedule.of(self, "rev", [t for t, _ in rows], [r for _, r in rows], _rev_steps=int(num_inference_steps),
                           _rev_direction=direction, _rev_from_code=bool(from_code),
                           _rev_strength=None if strength is None else N)

    def ilvr_schedule(self, num_inference_steps, eta=1.0, range_t=0):
        """ILVR reference-guided sampling (Choi et al., ICCV 2021, Algorithm 1) over this scheduler's `num_inference_steps`
        timesteps g[0] > ... > g[N-1], as the Schedule DenoiseEngine replays with afldm_ilvr_step.  For evaluation i, with
        ab = alphas_cumprod[g[i]] and ab' the next level (final_alpha_cumprod after the last):
          x' = the reverse step of repaint_schedule (eta = 1: DDPM's ancestral step, which the paper samples with)
          y' = sqrt(ab') ref + sqrt(1-ab') z_k        the reference noised to level t-1, as Algorithm 1 states (the authors'
                                                      public code noises it to level t); y' = ref on the last evaluation
          x_out = x' + w phi(y' - x'),  w = 1 while g[i] > range_t and 0 from there on (the paper's conditioning range)
        Draws per evaluation, in this order: z_k where w != 0 and its coefficient is not 0, z_u where sigma != 0 - one
        randn_tensor of the latent shape in the model's dtype each."""
        n = int(num_inference_steps)
        if self.config.prediction_type != "epsilon":
            raise NotImplementedError("afldm_amd.DDIMScheduler.ilvr_schedule implements epsilon prediction")
        self.set_timesteps(n)
        g = self._timesteps_host
        rows, draws = [], []
        for i, t in enumerate(g):
            last = i == n - 1
            ab = float(self.alphas_cumprod[t])
            ab_prev = float(self.final_alpha_cumprod) if last else float(self.alphas_cumprod[g[i + 1]])
            reverse = self._reverse_row(ab, ab_prev, eta)
            k0, k1 = (1.0, 0.0) if last else (math.sqrt(ab_prev), math.sqrt(1 - ab_prev))
            w = 1.0 if t > range_t else 0.0
            rows.append(reverse + (k0, k1, w, 0.0, 0.0))
            draws.append((w != 0.0 and k1 != 0.0, reverse[6] != 0.0))
        return Schedule.of(self, "ilvr", g, rows, draws, _ilvr_steps=n, _ilvr_eta=float(eta), _ilvr_range_t=int(range_t))

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' first")
        if self.config.clip_sample or self.config.prediction_type != "epsilon":
            raise NotImplementedError("afldm_amd.DDIMScheduler implements the reference's setting: "
                                      "epsilon prediction, clip_sample=False")
        if not sample.is_cuda:
            raise RuntimeError("afldm_amd.DDIMScheduler.step runs on MI355X tensors only (no CPU path)")
        c = self.coefficients(timestep)
        x = sample.to(torch.float32).contiguous()
        e = model_output.to(torch.float32).contiguous()
        if eta == 0.0:
            prev = ops.ddim_step_flat(x, e, c).to(sample.dtype)
        else:
            # diffusers DDIMScheduler.step with eta > 0 (the reference forwards `eta`, ldm_pipeline.py:38,96-101):
            # sigma_t = eta sqrt((1 - a_prev) / (1 - a_t) (1 - a_t / a_prev)); the direction coefficient becomes
            # sqrt(1 - a_prev - sigma_t^2) and sigma_t * noise is added (noise drawn like diffusers: randn_tensor with the
            # caller's generator, on the CPU for a CPU generator)
            sigma = float(eta) * self._variance(timestep) ** 0.5
            a_prev = c[2] * c[2]
            prev = ops.ddim_step_flat(x, e, (c[0], c[1], c[2], float(max(1.0 - a_prev - sigma * sigma, 0.0) ** 0.5)))
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` "
                                 "or `variance_noise` stays `None`.")
            if variance_noise is None:
                variance_noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device,
                                              dtype=model_output.dtype)
            prev = (prev + sigma * variance_noise.to(torch.float32)).to(sample.dtype)
        if not return_dict:
            return (prev,)
        return DDIMSchedulerOutput(prev_sample=prev)

    def __len__(self):
        return self.config.num_train_timesteps


def ffhq_ddim_scheduler():
    return DDIMScheduler.from_config(FFHQ_DDIM_CONFIG)
