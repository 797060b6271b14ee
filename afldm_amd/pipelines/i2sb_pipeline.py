"""I2SBLDMPipeline — surface of reference afldm/pipelines/i2sb_pipeline.py:17-78: the degraded
image is VAE-encoded and used as the INITIAL latent of the (unconditional) alias-free UNet; the
loop breaks before the last timestep (num_inference_steps - 1 UNet evaluations)."""
import torch

from ..schedulers.i2sb import I2SBScheduler
from .ldm_pipeline import MyLDMPipeline


class I2SBLDMPipeline(MyLDMPipeline):
    def __init__(self, vae, unet, scheduler: I2SBScheduler):
        super().__init__(vae, unet, scheduler)

    @torch.no_grad()
    def __call__(self, images, generator=None, is_ode=False, num_inference_steps=50, output_type="pil",
                 return_dict=True, reference_exact=True, latent_dtype=torch.float32, use_graph=True, **kwargs):
        """images: [B, 3, H, W] tensor in [-1, 1] (the reference's VaeImageProcessor.preprocess leaves
        such tensors unchanged).  Like the reference (i2sb_pipeline.py:43) the posterior sample of the start latent is
        drawn by latent_dist.sample() WITHOUT the caller's generator; reference_exact=False opts into drawing it from
        `generator` (seeded runs become reproducible end to end).

        latent_dtype: the dtype the latent is CARRIED in between UNet evaluations.  Default fp32 - a deliberate deviation
        from the reference for bf16 / fp16 UNets, where the reference stores the latent in the UNet's dtype
        (i2sb_pipeline.py:41) and loses 0.11 rel-RMS over the 99 evaluations to storage rounding alone
        (tests/golden/g16_r04_floor.npz); with an fp32 UNet both are the same thing.  `latent_dtype=None` reproduces the
        reference's storage (the latent stays in the UNet's dtype)."""
        if self.vae is None:
            raise NotImplementedError("I2SBLDMPipeline needs a VAE to encode the degraded image")
        start = self.vae.encode(images.to(device=self.device, dtype=self.unet.dtype)).latent_dist.sample(
            None if reference_exact else generator)
        latents = self._bridge(start * self.vae.config.scaling_factor, num_inference_steps, is_ode, generator,
                               latent_dtype=latent_dtype, use_graph=use_graph)
        return self._deliver(latents, output_type, return_dict)

    def _bridge(self, latents, steps, is_ode, generator, latent_dtype=torch.float32, use_graph=True):
        """steps - 1 UNet evaluations from the encoded degraded image towards the clean latent: the reference loop
        leaves before its last timestep (i2sb_pipeline.py:48-50).  With the latent carried in fp32 every form replays captured
        HIP graphs (use_graph): the deterministic, unclipped bridge (is_ode, clip_sample off - what scripts/shift_ldm_sr.py
        runs) on the DDIM kernel's linear form, the stochastic and / or clipped forms on afldm_sde_step, whose noise the engine
        draws with `generator` exactly as the loop below does (same randn_tensor calls, same order).  use_graph=False and
        latent_dtype=None run the eager loop below."""
        sched, unet = self.scheduler, self.unet
        if use_graph and latent_dtype == torch.float32 and latents.is_cuda and steps >= 2:
            from ..engine import cached_engine
            ode = sched.ode_schedule(steps) if is_ode else None
            if ode is not None:
                # the same captured-graph loop the DDIM sampler uses: the unclipped ODE update is the DDIM kernel's linear form
                return cached_engine(self, "_ode_engines", ode, latents.shape[0], True, unet).run(latents).to(latents.dtype)
            sde = sched.bridge_schedule(steps, is_ode)          # (engines cached apart from the unclipped ODE's)
            eng = cached_engine(self, "_sde_engines", sde, latents.shape[0], True, unet)
            draw = sde.drawer(generator, tuple(latents.shape), latents.device, torch.float32)
            return eng.run(latents, draw=draw).to(latents.dtype)
        sched.set_timesteps(steps)
        # The latent is carried in fp32 BETWEEN evaluations whatever the UNet's dtype (as DenoiseEngine does for DDIM): a
        # step of the 100-step bridge moves the latent by about one bf16 ulp, and a latent stored in bf16 - what the
        # reference does with a bf16 UNet (i2sb_pipeline.py:41; scheduler.step returns the sample's dtype) - loses 0.11
        # rel-RMS over the 99 evaluations to storage rounding alone (oracle measurement: tests/golden/g16_r04_floor.npz).
        # The UNet still sees its own dtype; the result is returned in the caller's dtype.  latent_dtype=None: the
        # reference's storage (the latent keeps the dtype it came in with).
        dtype = latents.dtype
        if latent_dtype is not None:
            latents = latents.to(latent_dtype)
        for t in self.progress_bar(sched._timesteps_host[:steps - 1]):
            prediction = unet(sched.scale_model_input(latents, t).to(unet.dtype), t).sample
            latents = sched.step(prediction, t, latents, is_ode=is_ode, generator=generator).prev_sample
        return latents.to(dtype)

    def panorama_latents(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: MultiDiffusion panoramas are defined for the unconditional sampler "
                                  "(MyLDMPipeline.panorama_latents); the bridge starts from an encoded image of the window's size")

    def panorama(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: MultiDiffusion panoramas are defined for the unconditional sampler "
                                  "(MyLDMPipeline.panorama); the bridge starts from an encoded image of the window's size")

    def outpaint_latents(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: outpainting is defined for the unconditional sampler "
                                  "(MyLDMPipeline.outpaint_latents); the bridge starts from an encoded image of the window's size")

    def outpaint(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: outpainting is defined for the unconditional sampler "
                                  "(MyLDMPipeline.outpaint); the bridge starts from an encoded image of the window's size")

    def hires_latents(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: high-resolution sampling is defined for the unconditional sampler "
                                  "(MyLDMPipeline.hires_latents); the bridge starts from an encoded image of the window's size")

    def hires(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: high-resolution sampling is defined for the unconditional sampler "
                                  "(MyLDMPipeline.hires); the bridge starts from an encoded image of the window's size")

    def img2img_latents(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: image-to-image sampling (SDEdit) is defined for the unconditional sampler "
                                  "(MyLDMPipeline.img2img_latents); the bridge has its own start, the encoded low-resolution image")

    def img2img(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: image-to-image sampling (SDEdit) is defined for the unconditional sampler "
                                  "(MyLDMPipeline.img2img); the bridge has its own start, the encoded low-resolution image")

    def cfg_latents(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: classifier-free guidance is defined for the class-conditional DDIM sampler "
                                  "(MyLDMPipeline.cfg_latents); the bridge's UNet is conditioned on its start image, not on a label")

    def cfg(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: classifier-free guidance is defined for the class-conditional DDIM sampler "
                                  "(MyLDMPipeline.cfg); the bridge's UNet is conditioned on its start image, not on a label")

    def _no_reversible(self, *args, **kwargs):
        raise NotImplementedError("I2SBLDMPipeline: the bit-reversible sampler is defined for the unconditional DDIM sampler "
                                  "(MyLDMPipeline.sample_reversible / invert_reversible); a reversible bridge is not implemented")

    sample_reversible = sample_reversible_latents = invert_reversible = _no_reversible
