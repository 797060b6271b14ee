"""SdeSchedule — scheduler-shaped view of a stochastic sampler for the graph-replayed engine (DenoiseEngine with
update_kind = "sde", afldm_sde_step).  Each step is one coefficient row and at most one noise tensor:

    x0 = clamp(p x + q eps, lo, hi);  x_out = a x + b x0 + d eps + c z

The rows come from the scheduler that owns the update (DDIMScheduler.stochastic_schedule, I2SBScheduler.bridge_schedule),
computed in float64 and rounded once to fp32.  The schedule also states which steps draw noise and how: exactly the
randn_tensor calls, in the same order, that the scheduler's eager `step()` makes, so that the engine can draw them from the
caller's generator before the captured graphs need them."""
import torch

from ..configs import FrozenConfig
from ..utils import randn_tensor


class SdeSchedule:
    update_kind = "sde"

    def __init__(self, config, timesteps, rows, draws, noise_dtype=None):
        """config: the owning scheduler's config plus the settings the rows depend on (an engine cache key); timesteps: one per
        step; rows: (p, q, lo, hi, a, b, d, c) per step, float64; draws: per step, whether the eager step draws a noise
        tensor; noise_dtype: the dtype of that draw (None: the model's dtype, what DDIMScheduler.step draws in)."""
        assert len(timesteps) == len(rows) == len(draws)
        self.config = FrozenConfig(config)
        self._timesteps_host = [int(t) for t in timesteps]
        self.rows = [tuple(float(v) for v in r) for r in rows]
        self.draws = tuple(bool(d) for d in draws)
        self.noise_dtype = noise_dtype
        self.init_noise_sigma = 1.0

    def set_timesteps(self, n=None, device=None):
        assert n in (None, len(self.rows)), "the schedule is fixed when it is made"

    def coefficient_table(self, device):
        """float32 [nsteps, 8] rows (p, q, lo, hi, a, b, d, c) for afldm_sde_step, rounded once from float64."""
        return torch.tensor(self.rows, dtype=torch.float64).to(torch.float32).to(device)

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
