"""MyLDMPipeline — surface of reference afldm/pipelines/ldm_pipeline.py:17-160 on MI355X.

`__call__(output_type='latent')` is the throughput entry point: the DDIM loop runs as a
replayed HIP graph (afldm_amd.engine.DenoiseEngine); other output types decode through the
(alias-free) AutoencoderKL of afldm_amd.models.vae."""
import inspect
import json
import os

import torch

from ..engine import cached_engine
from ..models.unet_2d import UNet2DModel
from ..schedulers.ddim import DDIMScheduler
from ..schedulers.dpmsolver import DPMSolverMultistepScheduler
from ..schedulers.schedule import Schedule
from ..utils import randn_tensor
from .pipeline_utils import DiffusionPipeline, ImagePipelineOutput


class MyLDMPipeline(DiffusionPipeline):
    def __init__(self, vae, unet: UNet2DModel, scheduler: DDIMScheduler):
        super().__init__()
        self.register_modules(vae=vae, unet=unet, scheduler=scheduler)

    @classmethod
    def from_pretrained(cls, path, **kw):
        """Local diffusers-format directory: unet/ (config.json + safetensors), scheduler/
        (scheduler_config.json), optional vae/.  There is no network access on the target boxes."""
        if not os.path.isdir(path):
            raise OSError(f"{path} is not a local directory (afldm_amd cannot download checkpoints)")
        unet = UNet2DModel.from_pretrained(path, subfolder="unet")
        with open(os.path.join(path, "scheduler", "scheduler_config.json")) as f:
            scheduler = DDIMScheduler.from_config(json.load(f))
        vae = None
        if os.path.isdir(os.path.join(path, "vae")):
            from ..models.vae import AutoencoderKL
            vae = AutoencoderKL.from_pretrained(path, subfolder="vae")
        return cls(vae, unet, scheduler)

    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, eta=0.0, num_inference_steps=50, latents=None,
                 output_type="pil", return_dict=True, use_graph=True, **kwargs):
        # DDIM, as the reference forces (ldm_pipeline.py:80), unless the caller opted into DPM-Solver(++): that one is
        # re-created from its own config, and `eta` does not apply to it (diffusers' accepts_eta)
        dpm = isinstance(self.scheduler, DPMSolverMultistepScheduler)
        sched_cls = DPMSolverMultistepScheduler if dpm else DDIMScheduler
        self.scheduler = sched_cls.from_config(self.scheduler.config)
        if latents is None:
            latents = randn_tensor((batch_size, self.unet.config.in_channels, self.unet.config.sample_size,
                                    self.unet.config.sample_size), generator=generator)
        if eta != 0.0 and not dpm and use_graph:
            # stochastic DDIM (reference ldm_pipeline.py:96-109 forwards eta to scheduler.step) on the captured graphs: the
            # engine draws every step's noise with the caller's generator - the randn_tensor calls of the loop below, in its
            # order - before the replays that read it.  The latent is carried in fp32 between steps, as for eta = 0; with a
            # bf16 UNet the loop below stores it in bf16 (the reference's storage), so the two differ by that rounding.
            sde = self.scheduler.stochastic_schedule(num_inference_steps, eta)
            eng = cached_engine(self, "_engines", sde, latents.shape[0], use_graph, self.unet)
            draw = sde.drawer(generator, tuple(latents.shape), self.unet.device, self.unet.dtype)
            latents = eng.run(latents, draw=draw).to(self.unet.dtype)
            return self._deliver(latents, output_type, return_dict)
        if eta != 0.0 and not dpm:
            # stochastic DDIM, use_graph=False: the eager loop, one scheduler.step per UNet evaluation
            self.scheduler.set_timesteps(num_inference_steps)
            latents = latents.to(device=self.unet.device, dtype=self.unet.dtype)
            for t in self.progress_bar(self.scheduler._timesteps_host):
                eps = self.unet(latents, t).sample
                latents = self.scheduler.step(eps, t, latents, eta=eta, generator=generator).prev_sample
            return self._deliver(latents, output_type, return_dict)
        # the engine is keyed on the schedule's key - the scheduler's class, CONFIG and step count - not on the scheduler
        # object, which is re-created on every call (like the reference, ldm_pipeline.py:80); it shows the current one
        eng = cached_engine(self, "_engines", self.scheduler.schedule(num_inference_steps), latents.shape[0], use_graph, self.unet)
        eng.scheduler = self.scheduler
        latents = eng.run(latents).to(self.unet.dtype)
        return self._deliver(latents, output_type, return_dict)

    def _deliver(self, latents, output_type, return_dict):
        """'latent' -> the latents; 'pt' -> decoded tensor in [-1, 1]; 'np' / 'pil' -> [0, 1] NHWC arrays / PIL images
        (wrapped in ImagePipelineOutput unless return_dict is False)."""
        if output_type == "latent":
            return latents
        if self.vae is None:
            raise NotImplementedError("this pipeline was built without a VAE: use output_type='latent'")
        decoded = self.vae.decode(latents.to(self.vae.dtype) / self.vae.config.scaling_factor).sample
        if output_type == "pt":
            return decoded
        arrays = (decoded / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()
        images = self.numpy_to_pil(arrays) if output_type == "pil" else arrays
        return ImagePipelineOutput(images=images) if return_dict else (images,)

    def _inversion_rows(self):
        """(timestep, (mu_prev, sigma_prev, mu, sigma)) per step of the inversion over the scheduler's current timesteps, reversed:
        latent <- mu (latent - sigma_prev eps) / mu_prev + sigma eps (reference ldm_pipeline.py:133-160) - the DDIM update kernel's
        linear form with (sqrt a_t, sqrt(1 - a_t)) := (mu_prev, sigma_prev) and (sqrt a_prev, sqrt(1 - a_prev)) := (mu, sigma)."""
        ts = list(reversed(self.scheduler._timesteps_host))
        ac = self.scheduler.alphas_cumprod
        rows = []
        for i, t in enumerate(ts):
            a_t = ac[t]
            a_prev = ac[ts[i - 1]] if i > 0 else self.scheduler.final_alpha_cumprod
            rows.append((t, (float(a_prev ** 0.5), float((1 - a_prev) ** 0.5), float(a_t ** 0.5), float((1 - a_t) ** 0.5))))
        return rows

    def inversion_schedule(self):
        """_inversion_rows as the Schedule DenoiseEngine replays with afldm_ddim_step (timesteps ascending)."""
        rows = self._inversion_rows()
        ts = [t for t, _ in rows]
        return Schedule.of(self.scheduler, "ddim", ts, [c for _, c in rows], _inversion_timesteps=tuple(ts))

    @torch.no_grad()
    def ddim_inversion(self, latent, bar=True, use_graph=True):
        """Deterministic DDIM inversion over reversed timesteps (reference ldm_pipeline.py:133-160).  use_graph (fp32 latents on the
        GPU, plain attention processors): the loop replays DenoiseEngine's captured graphs over the inversion's coefficient rows;
        otherwise - bf16 latents, which the reference carries in their own dtype between steps, or a UNet with cross-frame
        processors installed - the eager loop below."""
        from .. import ops
        if isinstance(self.scheduler, DPMSolverMultistepScheduler):
            raise NotImplementedError("ddim_inversion needs a DDIMScheduler: DPM-Solver inversion is not implemented")
        sched = self.inversion_schedule()
        if (use_graph and latent.is_cuda and latent.dtype == torch.float32 and len(sched.rows) >= 1
                and tuple(latent.shape[1:]) == (self.unet.config.in_channels, self.unet.config.sample_size, self.unet.config.sample_size)
                and all(type(m.processor).__name__ == "AttnProcessor2_0" for m in self.unet.modules() if hasattr(m, "processor"))):
            return cached_engine(self, "_inv_engines", sched, latent.shape[0], True, self.unet).run(latent).to(latent.dtype)
        rows = list(zip(sched.timesteps, sched.rows))
        it = self.progress_bar(rows) if bar else rows
        for t, coef in it:
            eps = self.unet(latent, t).sample
            latent = ops.ddim_step_flat(latent.float().contiguous(), eps.float().contiguous(), coef).to(latent.dtype)
        return latent
