"""Schedule — what a sampler hands the graph-replayed engine (afldm_amd/engine.py): one timestep and one coefficient row per
UNet evaluation, fixed when it is made.  `kind` names the update kernel that reads the rows:

    "ddim"  (c0, c1, c2, c3):            x0 = (x - c1 eps) / c0;  x_out = c2 x0 + c3 eps                  afldm_ddim_step
    "dpm"   (p, q, a, b0, b1, b2, 0, 0): m0 = p x + q eps;  x_out = a x + b0 m0 + b1 m1 + b2 m2           afldm_dpm_step
    "sde"   (p, q, lo, hi, a, b, d, c):  x0 = clamp(p x + q eps, lo, hi);  x_out = a x + b x0 + d eps + c z   afldm_sde_step
    "seeded" the "sde" row, float for float, with z made in the update's registers from (the sample's seed, the step ordinal,
            the element) by a counter-based generator - no draws, no noise buffer:
            t = rn(p x) + rn(q eps);  x0 = clamp(t, lo, hi);  x_out = ((rn(a x) + rn(b x0)) + rn(d eps)) + rn(c z)   afldm_seeded_step
    "repaint" (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0):  x0 = clamp(p x + q eps, lo, hi);  unknown = a x0 + b eps + c z_u;
            y = m (k0 known + k1 z_k) + (1 - m) unknown;  x_out = u0 y + u1 z_b                           afldm_repaint_step
    "ilvr"  (p, q, lo, hi, a, b, c, k0, k1, w, 0, 0):  x0 = clamp(p x + q eps, lo, hi);  xp = a x0 + b eps + c z_u;
            x_out = xp + w L ((k0 ref + k1 z_k) - xp) L^T, per plane                                      afldm_ilvr_step
    "pano"  (p, q, lo, hi, a, b, d, c):  the "sde" row applied per window of a larger canvas and averaged over the windows that
            cover an element (MultiDiffusion):  x_out = a x + b mean_k x0_k + d mean_k eps_k + c z                afldm_pano_step
    "outpaint"  the "repaint" row, float for float, applied on a canvas: x0 per window, then RePaint's update with the means over the
            covering windows in x0's and eps's place, the known content, the mask and the three noise slots canvas-shaped:
            unknown = a mean_k x0_k + b mean_k eps_k + c z_u;  the rest as "repaint"                    afldm_pano_repaint_step
    "hires" (p, q, lo, hi, a, b, c, k0, k1, r, g, f):  high-resolution sampling on a canvas of scale x the window (after DemoFusion):
            the local windows' means as "pano", mixed by g with the prediction of the dilated window through the element, one
            reverse step, the skip residual r towards the noised upsampled reference, and the dilated views of the next UNet input
            low-passed by f:  x0m = (1 - g) mean_k x0_k + g x0_g;  em = (1 - g) mean_k eps_k + g eps_g;  xp = a x0m + b em + c z_u;
            x_out = r (k0 ref + k1 eps_ref) + (1 - r) xp;  dilated input = x_out + f (L x_out L^T - x_out)       afldm_hires_step
    "pag"   (p, q, lo, hi, a, b, d, c, s, phi, 0, 0):  perturbed-attention guidance on a batch of 2 B, e the UNet's output and e_p
            the perturbed UNet's:  g = e + s (e - e_p);  phi != 0: g <- g (phi std(e) / std(g) + 1 - phi) per sample;  then the
            "sde" row applied to g:  x0 = clamp(p x + q g, lo, hi);  x_out = a x + b x0 + d g + c z          afldm_pag_step
    "sag"   the "pag" row, float for float (s = sag_scale): self-attention guidance, two DEPENDENT evaluations per step - e, then
            e_d on the input degraded where the attention mass of one site exceeds 1 (afldm_sag_degrade reads p and q of the
            row) - and the same guided update with e_d in e_p's place                                        afldm_pag_step
    "cfg"   the "pag" row with s = guidance_scale - 1: classifier-free guidance over class labels on a batch of 2 B, e the output on
            the conditional rows and e_p the output on the unconditional rows (CFGEngine)                  afldm_pag_step
    "sdedit" (p, q, lo, hi, a, b, c, k0, k1, thr, 0, 0):  image-to-image sampling (SDEdit) with a per-element change map
            (Differential Diffusion):  x0 = clamp(p x + q eps, lo, hi);  xp = a x0 + b eps + c z_u;  held = k0 orig + k1 z, z the
            run's ONE fixed noise;  x_out = (cmap <= thr) ? held : xp - a select, not a blend         afldm_sdedit_step
    "seeded_sdedit"  the "sdedit" row, float for float, for the slot sampler (EditSlotEngine): both of its noises are made in the
            update's registers from the request's seed - z_u is noise slot 0 at the row's ordinal, the run's one fixed noise z is
            slot 1 at ordinal 0 - and the original and the change map are the slot's own planes; no draws:
            t = rn(p x) + rn(q eps);  x0 = clamp(t, lo, hi);  xp = (rn(a x0) + rn(b eps)) + rn(c z_u);  held = rn(k0 orig) + rn(k1 z);
            x_out = (cmap <= thr) ? held : xp                                                              afldm_slot_step_edit
    "seeded_repaint"  the "repaint" row, float for float, likewise: z_k, z_u, z_b are the noise slots 0, 1, 2 at the row's ordinal,
            the known latents and the mask the slot's own planes; no draws:  x0 as above;  unknown = (rn(a x0) + rn(b eps)) + rn(c z_u);
            knownp = rn(k0 known) + rn(k1 z_k);  y = rn(m knownp) + rn(rn(1 - m) unknown);  x_out = rn(u0 y) + rn(u1 z_b)   afldm_slot_step_edit
    "rev"   (cx, ce, sign, boot):  the bit-reversible sampler (two-step DDIM after BDIA, gamma = 1) on a pair (far, near) of int64
            latents on the grid 2^-32:  f = boot ? near : far;  x = rn_f32(near) 2^-32;  q = rn_i64(fl32(fl32(cx x) + fl32(ce eps)) 2^32);
            far <- near;  near <- f + sign q - integer arithmetic, so the same row with the other sign undoes it    afldm_rev_step

The rows come from the scheduler that owns the update (DDIMScheduler.schedule / stochastic_schedule / seeded_schedule,
DDIMScheduler.seeded_sdedit_schedule / seeded_repaint_schedule / repaint_schedule / ilvr_schedule / panorama_schedule / pag_schedule / sag_schedule / outpaint_schedule / hires_schedule / sdedit_schedule / reversible_schedule, DPMSolverMultistepScheduler.schedule, I2SBScheduler.ode_schedule / bridge_schedule,
MyLDMPipeline.inversion_schedule) as Python floats and are rounded once to fp32 by `table`.  An "sde" schedule also states which
steps draw noise and how: exactly the randn_tensor calls, in the same order, that the scheduler's eager `step()` makes, so that
the engine can draw them from the caller's generator before the captured graphs need them.  A "repaint" schedule has up to
three draws per step and states them per slot: `draws[k]` is (z_k, z_u, z_b), drawn in that order; an "ilvr" schedule has up
to two, (z_k, z_u).  A "pano" schedule draws one canvas-shaped tensor per step, and only where the row's c is not 0; an "outpaint" schedule draws as
"repaint" does, canvas-shaped; a "hires" schedule draws as "pano" does; an "sdedit" schedule draws one latent-shaped z_u per step, only where
the row's c is not 0 (its fixed noise z is a per-run tensor like the original, not a draw of a step).  `key` identifies everything the rows were computed from; the engine
cache (engine.cached_engine) compares it, so two schedules with equal keys must replay the same graph."""
from dataclasses import dataclass

import torch

from ..configs import FrozenConfig
from ..utils import randn_tensor

# kind -> (row width, noise slots per step, may a step draw): the one place that states them.  Several slots: `draws` is per slot
KINDS = {"ddim": (4, 1, False), "dpm": (8, 1, False), "sde": (8, 1, True), "repaint": (12, 3, True), "ilvr": (12, 2, True),
         "pano": (8, 1, True), "pag": (12, 1, True), "sag": (12, 1, True), "outpaint": (12, 3, True),
         "hires": (12, 1, True), "sdedit": (12, 1, True), "rev": (4, 1, False), "cfg": (12, 1, True), "seeded": (8, 1, False),
         "seeded_sdedit": (12, 2, False), "seeded_repaint": (12, 3, False)}
ROW_WIDTH, NOISE_SLOTS = {k: v[0] for k, v in KINDS.items()}, {k: v[1] for k, v in KINDS.items() if v[2]}      # derived views
_MADE = {}          # key -> Schedule: the rows are ~0.1 ms of scalar tensor arithmetic each, and a sampler asks per call


@dataclass(frozen=True, eq=False)
class Schedule:
    kind: str
    timesteps: tuple
    rows: tuple
    draws: tuple
    noise_dtype: object
    init_noise_sigma: float
    config: FrozenConfig          # the owner's config plus the settings: what `key` is the hashable form of
    key: tuple

    @classmethod
    def of(cls, owner, kind, timesteps, rows, draws=None, noise_dtype=None, **settings):
        """owner: the scheduler whose config the rows are computed from; settings: whatever else they depend on (the step
        count, eta, is_ode, ...); rows: one per timestep, or a function of the timestep that is only called when no schedule
        with this key has been made yet; draws: per step, whether the eager step draws a noise tensor, or for a kind of several
        slots one bool per slot (KINDS); noise_dtype: the dtype of that draw (None: the model's dtype, as DDIMScheduler.step)."""
        config = FrozenConfig(dict(owner.config, **settings))
        key = (type(owner).__name__, tuple(sorted((k, repr(v)) for k, v in config.items())))
        if key in _MADE:
            return _MADE[key]
        timesteps = tuple(int(t) for t in timesteps)
        if callable(rows):
            rows = [rows(t) for t in timesteps]
        rows = tuple(tuple(float(v) for v in r) for r in rows)
        width, nslots, may_draw = KINDS[kind]
        if nslots > 1:
            draws = tuple(tuple(bool(v) for v in d) for d in draws) if draws is not None else ((False,) * nslots,) * len(rows)
            assert all(len(d) == nslots for d in draws)
        else:
            draws = tuple(bool(d) for d in draws) if draws is not None else (False,) * len(rows)
        drawn = any(any(d) if isinstance(d, tuple) else d for d in draws)
        assert len(timesteps) == len(rows) == len(draws) and all(len(r) == width for r in rows) and (may_draw or not drawn)
        while len(_MADE) >= 64:
            del _MADE[next(iter(_MADE))]          # the oldest: a schedule just made outlives the next 63, whoever makes them
        made = _MADE[key] = cls(kind, timesteps, rows, draws, noise_dtype, float(owner.init_noise_sigma), config, key)
        return made

    def table(self, device):
        """float32 [nsteps, row width] device table, each entry rounded once from the Python float."""
        return torch.tensor(self.rows, dtype=torch.float64).to(torch.float32).to(device)

    # read-only spellings of the scheduler-shaped views this type replaced; tests/test_sde_host.py checks every row through them
    update_kind = property(lambda self: self.kind)
    _timesteps_host = property(lambda self: list(self.timesteps))
    coefficient_table = table

    def slots(self, k):
        """The noise slots step k draws, in drawing order: a subset of range(KINDS[kind][1])."""
        d = self.draws[k]
        return tuple(j for j, on in enumerate(d) if on) if isinstance(d, tuple) else ((0,) if d else ())

    def draw_noise(self, shape, generator, device, model_dtype):
        """One step's noise, as the eager step draws it: randn_tensor(shape, generator, device, dtype).  With a CPU generator
        the values do not depend on `device` (randn_tensor draws on the CPU and moves the result)."""
        return randn_tensor(shape, generator=generator, device=device, dtype=self.noise_dtype or model_dtype)

    def drawer(self, generator, shape, device, model_dtype):
        """The `draw` callable DenoiseEngine.run takes: each call is the next step's draw_noise with the caller's generator (a
        torch.Generator, a list of them - one per sample - or None for the device's default generator).  With CPU generators it
        returns the CPU tensor, which the engine stages through pinned memory; otherwise the draw runs on `device`."""
        g0 = generator[0] if isinstance(generator, list) and generator else generator
        where = torch.device("cpu") if isinstance(g0, torch.Generator) and g0.device.type == "cpu" else device
        return lambda: self.draw_noise(shape, generator, where, model_dtype)
