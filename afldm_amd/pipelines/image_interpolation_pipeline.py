"""LDMInterpolationPipeline — image interpolation of reference afldm/pipelines/image_interpolation_pipeline.py:284-766 on the
unconditional UNet this project serves (the text-prompt and classifier-free-guidance parts drop out):

  1. both images -> sample_size * vae_scale_factor, [-1, 1];
  2. image2latent (:270-282): the MEAN of the VAE posterior times scaling_factor;
  3. DDIM inversion of each latent (:232-268; the reference's processors store nothing it reads: plain processors here);
  4. frame 0 / n-1 = the inverted latents, frame i = slerp(frame 0, frame n-1, linspace(0, 1, n)[i]) (warp_method 3); with
     warp_method 0 / 1 / 2 and the caller's optical flow (flows=) each endpoint's noise is first forward-warped along the flow
     scaled by the frame's fraction (:556-599; initial_frames, shift_utils/flow_utils.py);
  5. two STORE passes of the full schedule, endpoint 0 into slot 0, endpoint 1 into slot 1 (:604-652);
  6. the LOAD pass (:668-735): at every step each frame f attends to both stored passes, blended by alpha = f / (n - 1),
     then one DDIM step (eta 0) advances all frames;
  7. decode every frame.

use_graph=True (default) runs 3 as one batch-2 graph run, 5 as ONE batch-2 graph (AttnState.PAIR), 6 as one graph over all
n frames with a per-sample alpha buffer (each attention = one afldm_attention_interp launch over both cached K / V^T pairs)
and 7 as one batched decode; the captures are cached on the pipeline, later calls replay.  use_graph=False follows the
reference statement by statement: batch-1 passes, a per-frame LOAD with a host alpha, the non-cached processors, a per-frame
warp (the graph path warps all frames of an endpoint in one afldm_flow_splat call).
DESIGN.md sections 12 and 13 list the deviations from the reference script."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from ..schedulers.ddim import DDIMScheduler
from .cross_frame_attn import (AttnState, CrossFrameAttnProcessor, eager_pass, get_unet_attn_processors,
                               set_unet_attn_processor)
from .ldm_pipeline import MyLDMPipeline


def _arc_weights(cos_omega, t):
    """Weights (w0, w1) of spherical interpolation at fraction t for the angle whose cosine is `cos_omega` (float64 0-d
    tensors): w0 = sin((1 - t) omega) / sin omega, w1 = sin(t omega) / sin omega, with (1 - t) omega evaluated as
    omega - t omega."""
    omega = torch.arccos(cos_omega)
    t_omega = omega * t
    sin_omega = torch.sin(omega)
    return torch.sin(omega - t_omega) / sin_omega, torch.sin(t_omega) / sin_omega


@torch.no_grad()
def slerp(a, b, t):
    """Spherical interpolation between the tensors a and b at fraction t, the arithmetic of the reference's helper
    (image_interpolation_pipeline.py:68-108): everything in float64, the cosine of the angle between the flattened tensors
    clamped to [-1 + 1e-7, 1 - 1e-7] (parallel / antiparallel inputs stay finite), the result returned in fp16 for fp16
    inputs and in fp32 for every other dtype."""
    out_dtype = torch.float16 if a.dtype == torch.float16 else torch.float32
    a64, b64 = a.double(), b.double()
    cos_omega = torch.sum(a64 * b64) / (torch.linalg.norm(a64) * torch.linalg.norm(b64))
    w0, w1 = _arc_weights(cos_omega.clamp(-1 + 1e-7, 1 - 1e-7), t)
    return (a64 * w0 + b64 * w1).to(out_dtype)


def interp_alphas(num_frames):
    """(slerp fractions, LOAD blend weights) of an n-frame call.  They differ, as in the reference: the slerp takes
    torch.linspace(0, 1, n) in fp32 (:536), the blend the Python float f / (n - 1) (:680)."""
    return [float(a) for a in torch.linspace(0, 1, num_frames)], [f / (num_frames - 1) for f in range(num_frames)]


def check_interp_args(scheduler, num_frames, warp_method, flows=None, size=None):
    """The calls LDMInterpolationPipeline refuses (before any work).  flows: the caller's (fwd_flow, bwd_flow), each
    [1, 2, size, size] (size = the image side, checked when given)."""
    if warp_method != 3 and flows is None:
        raise NotImplementedError(f"warp_method={warp_method} warps the inverted noise along optical flow, which needs the GMFlow "
                                  "model: it is not available here; pass flows=(fwd_flow, bwd_flow) from any estimator, or use "
                                  "warp_method=3 (slerp of the inverted endpoints)")
    if warp_method not in (0, 1, 2, 3):
        raise ValueError(f"warp_method must be 0, 1, 2 or 3, got {warp_method!r}")
    if flows is not None:
        if not isinstance(flows, (tuple, list)) or len(flows) != 2:
            raise ValueError("flows must be the pair (fwd_flow, bwd_flow)")
        for name, f in zip(("fwd_flow", "bwd_flow"), flows):
            if not torch.is_tensor(f) or f.dim() != 4 or tuple(f.shape[:2]) != (1, 2) or f.shape[2] != f.shape[3] or \
                    (size is not None and f.shape[2] != size):
                raise ValueError(f"{name} must be a tensor [1, 2, S, S] at the image size S" + (f" = {size}" if size else "") +
                                 f", got {tuple(f.shape) if torch.is_tensor(f) else type(f).__name__}")
    if not isinstance(num_frames, (int, np.integer)) or num_frames < 2:
        raise ValueError(f"num_frames must be an integer >= 2 (the two endpoints are frames), got {num_frames!r}")
    if not isinstance(scheduler, DDIMScheduler):
        raise NotImplementedError(f"image interpolation samples with DDIM (inversion + cross-frame STORE / LOAD passes): a "
                                  f"pipeline whose scheduler is a {type(scheduler).__name__} is not supported")


class LDMInterpolationPipeline(MyLDMPipeline):
    """Two-image interpolation with the interpolating cross-frame attention.  Build it with from_pretrained(dir) (as
    MyLDMPipeline) or from another pipeline's modules: LDMInterpolationPipeline(**ldm_pipeline.components)."""

    def __init__(self, vae, unet, scheduler, flow_model=None):
        """flow_model: an optional flow estimator of shift_utils.flow_estimation (PyramidLKFlow).  With one, warp_method
        0 / 1 / 2 without flows= estimate the flow between the two images; without one (the default) nothing changes."""
        super().__init__(vae, unet, scheduler)
        self.flow_model = flow_model            # not a registered module: `components` stays (vae, unet, scheduler)

    @property
    def vae_scale_factor(self):
        return 2 ** (len(self.vae.config.block_out_channels) - 1)

    def _estimated_flows(self, image1, image2, timings=None):
        """(the two preprocessed images, (fwd_flow, bwd_flow) from predict_flow(self.flow_model, ...) on them).  With a timings
        dict the estimate's wall time goes to 'flow_s' (it runs before the phases 'total_s' covers)."""
        import time
        from ..shift_utils.flow_estimation import predict_flow
        size = self.unet.config.sample_size * self.vae_scale_factor
        images = [self._image(im, size) for im in (image1, image2)]
        if timings is not None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        fwd_flow, _, bwd_flow, _ = predict_flow(self.flow_model, *(x.to(self.unet.device) for x in images))
        if timings is not None:
            torch.cuda.synchronize()
            timings["flow_s"] = time.perf_counter() - t0
        return images, (fwd_flow, bwd_flow)

    def _image(self, image, size):
        """PIL image / path -> [1, 3, size, size] in [-1, 1] (Lanczos resize, diffusers VaeImageProcessor's default); a [-1, 1]
        tensor [1, 3, H, W] is resized (bilinear, antialiased) only when it is not size x size already."""
        from PIL import Image
        if isinstance(image, (str, os.PathLike)):
            image = Image.open(image)
        if isinstance(image, Image.Image):
            img = image.convert("RGB")
            if img.size != (size, size):
                img = img.resize((size, size), Image.LANCZOS)
            return torch.from_numpy(np.asarray(img, dtype=np.float32) / 127.5 - 1.0).permute(2, 0, 1)[None]
        if torch.is_tensor(image):
            if image.ndim != 4 or tuple(image.shape[:2]) != (1, 3):
                raise ValueError(f"an image tensor must be [1, 3, H, W] in [-1, 1], got {tuple(image.shape)}")
            x = image.detach().float().cpu()
            if tuple(x.shape[-2:]) != (size, size):
                x = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False, antialias=True)
            return x
        raise TypeError(f"an image is a PIL image, a path or a [1, 3, H, W] tensor, got {type(image).__name__}")

    @torch.no_grad()
    def image2latent(self, image):
        """Reference :270-282: the posterior MEAN (not a sample) times scaling_factor."""
        return self.vae.encode(image.to(device=self.vae.device, dtype=self.vae.dtype)).latent_dist.mean * self.vae.config.scaling_factor

    @torch.no_grad()
    def __call__(self, image1, image2, num_frames=17, num_inference_steps=50, warp_method=3, enable_interp=True,
                 output_type="pil", return_dict=True, use_graph=True, timings=None, flows=None, generator=None):
        """Returns the num_frames frames (output_type 'latent' / 'pt' / 'np' / 'pil', as MyLDMPipeline).  enable_interp=False
        keeps the reference's other branch: intermediate frames start from endpoint 0 and every frame attends to pass 0 only.
        timings: a dict that receives the wall time of the VAE ('vae_s'), the UNet passes ('unet_s'), the rest ('other_s') and
        'total_s' (synchronises at the phase boundaries; off when None).
        warp_method 0 / 1 / 2 (reference :556-599) start the intermediate frames from the inverted noise warped along
        flows = (fwd_flow, bwd_flow), each [1, 2, S, S] at the image size in the convention of the reference's predict_flow
        (channel 0 = x: the output of a GMFlow-style estimator as it is); generator seeds their random draws (the fill of
        disoccluded pixels, method 1's noise up-sampling).  warp_method 3 uses neither.  On a pipeline built with flow_model=,
        flows=None lets it estimate them from the two preprocessed images (shift_utils.flow_estimation.predict_flow)."""
        from ..harness import _Clock
        images = None
        if self.flow_model is not None and flows is None and warp_method in (0, 1, 2) and self.vae is not None:
            check_interp_args(self.scheduler, num_frames, 3)      # num_frames and the scheduler are refused before any work
            images, flows = self._estimated_flows(image1, image2, timings)      # then exactly as if the caller had passed them
        check_interp_args(self.scheduler, num_frames, warp_method, flows,
                          self.unet.config.sample_size * self.vae_scale_factor if self.vae is not None else None)
        if self.vae is None:
            raise NotImplementedError("image interpolation encodes its two images: this pipeline was built without a VAE")
        clock = _Clock(timings)
        unet, n = self.unet, int(num_frames)
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        size = unet.config.sample_size * self.vae_scale_factor
        if images is None:
            images = [self._image(im, size) for im in (image1, image2)]
        fracs, weights = interp_alphas(n)
        if not enable_interp:
            weights = [0.0] * n           # pass 0 only: alpha 0 is exactly the single-source attention
        clock.lap("other_s")
        warp = None if warp_method == 3 else (warp_method, flows, generator)
        if use_graph:
            latents = self._graph_frames(images, n, num_inference_steps, fracs, weights, enable_interp, clock, warp)
        else:
            latents = self._eager_frames(images, n, num_inference_steps, fracs, weights, enable_interp, clock, warp)
        out = self._deliver(latents, output_type, return_dict)
        clock.lap("vae_s")
        clock.done()
        return out

    def _frames(self, z0, z1, n, fracs, enable_interp):
        """Step 4: [n, C, H, W] initial latents from the two inverted ones (reference :551-599, warp_method 3)."""
        latents = torch.empty((n,) + tuple(z0.shape[1:]), dtype=z0.dtype, device=z0.device)
        latents[0], latents[-1] = z0[0], z1[0]
        for i in range(1, n - 1):
            latents[i] = slerp(latents[0], latents[-1], fracs[i]) if enable_interp else latents[0]
        return latents

    @torch.no_grad()
    def initial_frames(self, z0, z1, num_frames, warp_method, flows, generator=None, enable_interp=True, batched=True):
        """Step 4 with warp_method 0 / 1 / 2 (reference :462-471, :551-599): the [n, C, h, w] initial latents from the inverted
        endpoints z0, z1 [1, C, h, w] and flows = (fwd_flow, bwd_flow) [1, 2, S, S] (channel 0 = x, S = h * ds with
        ds = vae_scale_factor, the reference's constant 8 for the AF-VAE).
          0: ideal up-sampling by ds, forward warp along alpha * fwd_flow (endpoint 0) / (1 - alpha) * bwd_flow (endpoint 1),
             disoccluded pixels from ONE background draw for both endpoints, every ds-th pixel, slerp;
          1: upsample_noise + continuous_noise_fwd_warp (a fresh draw per frame and endpoint);
          2: the latents themselves along the nearest-decimated flows / ds, no fill (element 0 of forward_flow_warp's pair).
        batched=False is the reference loop, frame by frame through shift_utils.flow_utils; batched=True makes the same random
        draws in the same order first and then one afldm_flow_splat call per endpoint over all frames."""
        from ..af_libs.ideal_lpf import UpsampleRFFT
        from ..shift_utils import flow_utils as fu
        from ..utils import randn_tensor
        n, ds, dev = int(num_frames), self.vae_scale_factor, z0.device
        check_interp_args(self.scheduler, n, warp_method, flows, z0.shape[-1] * ds)
        fracs = interp_alphas(n)[0]
        if warp_method == 3 or n == 2:
            return self._frames(z0, z1, n, fracs, enable_interp)
        latents = torch.empty((n,) + tuple(z0.shape[1:]), dtype=z0.dtype, device=dev)
        latents[0], latents[-1] = z0[0], z1[0]
        # [W, H] -> [H, W] (:462-463): channel 0 becomes the row displacement
        f_flow, b_flow = (torch.flip(f.to(device=dev, dtype=torch.float32), (1,)).contiguous() for f in flows)
        f_flow_ds = F.interpolate(f_flow / ds, scale_factor=1 / ds, mode="nearest")
        b_flow_ds = F.interpolate(b_flow / ds, scale_factor=1 / ds, mode="nearest")
        alphas = torch.tensor(fracs, dtype=torch.float32)
        a_fwd, a_bwd = alphas[1:-1], (1 - alphas)[1:-1]            # fp32, as the reference's `alpha` and `1 - alpha` tensors
        draw = lambda like: randn_tensor(tuple(like.shape), generator=generator, device=dev, dtype=like.dtype)
        if warp_method != 1:
            up = UpsampleRFFT(ds)
            hi0, hi1 = up(latents[0].unsqueeze(0)), up(latents[-1].unsqueeze(0))
        else:
            hi0 = fu.upsample_noise(latents[0].unsqueeze(0), ds, generator=generator)
            hi1 = fu.upsample_noise(latents[-1].unsqueeze(0), ds, generator=generator)
        occ_bg = draw(hi0)                  # occ_bg2 = occ_bg1 (:566-567); drawn for every method, as the reference does
        if batched:
            if warp_method == 0:
                w1 = fu.forward_flow_warp_frames(hi0, f_flow, a_fwd, ds=ds, fill=occ_bg)[0]
                w2 = fu.forward_flow_warp_frames(hi1, b_flow, a_bwd, ds=ds, fill=occ_bg)[0]
            elif warp_method == 1:
                fills = [draw(hi0) for _ in range(2 * (n - 2))]            # frame by frame, endpoint 0 then endpoint 1
                w1 = fu.forward_flow_warp_frames(hi0, f_flow, a_fwd, ds=ds, pool=True, fill=torch.cat(fills[0::2]))[0]
                w2 = fu.forward_flow_warp_frames(hi1, b_flow, a_bwd, ds=ds, pool=True, fill=torch.cat(fills[1::2]))[0]
            else:
                w1 = fu.forward_flow_warp_frames(latents[0].unsqueeze(0), f_flow_ds, a_fwd)[0]
                w2 = fu.forward_flow_warp_frames(latents[-1].unsqueeze(0), b_flow_ds, a_bwd)[0]
        for i in range(1, n - 1):
            if batched:
                warped_1, warped_2 = w1[i - 1], w2[i - 1]
            elif warp_method == 0:
                alpha = alphas[i].to(dev)
                warped_1, tmp_occ = fu.forward_flow_warp(hi0, f_flow * alpha)
                warped_1 = (warped_1 * (1 - tmp_occ) + tmp_occ * occ_bg)[0, :, ::ds, ::ds]
                warped_2, tmp_occ = fu.forward_flow_warp(hi1, b_flow * (1 - alpha))
                warped_2 = (warped_2 * (1 - tmp_occ) + tmp_occ * occ_bg)[0, :, ::ds, ::ds]
            elif warp_method == 1:
                alpha = alphas[i].to(dev)
                warped_1 = fu.continuous_noise_fwd_warp(hi0, f_flow, alpha, ds, generator=generator)[0]
                warped_2 = fu.continuous_noise_fwd_warp(hi1, b_flow, 1 - alpha, ds, generator=generator)[0]
            else:
                alpha = alphas[i].to(dev)
                warped_1 = fu.forward_flow_warp(latents[0].unsqueeze(0), f_flow_ds * alpha)[0][0]
                warped_2 = fu.forward_flow_warp(latents[-1].unsqueeze(0), b_flow_ds * (1 - alpha))[0][0]
            latents[i] = slerp(warped_1, warped_2, fracs[i]) if enable_interp else warped_1
        return latents

    def _graph_frames(self, images, n, steps, fracs, weights, enable_interp, clock, warp=None):
        unet = self.unet
        lat = self.image2latent(torch.cat(images, 0)).float()
        clock.lap("vae_s")
        self.scheduler.set_timesteps(steps, device=unet.device)
        inv = self.ddim_inversion(lat, bar=False)            # both endpoints: one batch-2 run of the captured inversion graph
        clock.lap("unet_s")
        if warp is None:
            latents = self._frames(inv[0:1], inv[1:2], n, fracs, enable_interp)
        else:
            latents = self.initial_frames(inv[0:1], inv[1:2], n, *warp, enable_interp=enable_interp, batched=True)
        clock.lap("other_s")            # slerp, and with warp_method 0-2 the up-sampling, the draws and the warp: not UNet time
        out = self._graph_passes(inv, latents, steps, weights)
        clock.lap("unet_s")
        return out.to(unet.dtype)

    def _graph_passes(self, ends, latents, steps, weights):
        """Steps 5-6 on replayed graphs: the STORE pass of both endpoints `ends` [2, C, H, W] as one batch-2 graph (endpoint s ->
        slot s), then the LOAD pass of all frames `latents` [n, C, H, W] with blend weights `weights` (n floats).  Returns the
        fp32 latents; the caller's attention processors are restored."""
        from ..harness import _sampler
        smp = _sampler(self, DDIMScheduler.from_config(self.scheduler.config).schedule(steps), interp=True)
        previous = smp.install()
        try:
            smp.run(ends, load=False)
            return smp.run(latents, load=True, alpha=weights)
        finally:
            set_unet_attn_processor(self.unet, dict(previous))

    def _eager_frames(self, images, n, steps, fracs, weights, enable_interp, clock, warp=None):
        unet, sched = self.unet, self.scheduler
        lats = [self.image2latent(x) for x in images]
        clock.lap("vae_s")
        sched.set_timesteps(steps, device=unet.device)
        inv = [self.ddim_inversion(z.to(unet.dtype), bar=False, use_graph=False) for z in lats]
        clock.lap("unet_s")
        if warp is None:
            latents = self._frames(inv[0], inv[1], n, fracs, enable_interp)
        else:
            latents = self.initial_frames(inv[0], inv[1], n, *warp, enable_interp=enable_interp, batched=False)
        clock.lap("other_s")
        out = self._eager_passes(latents, steps, weights, enable_interp)
        clock.lap("unet_s")
        return out

    def _eager_passes(self, latents, steps, weights, enable_interp=True):
        """Steps 5-6 as the reference runs them (:604-735): batch-1 STORE passes of frame 0 (slot 0) and frame n-1 (slot 1) on the
        non-cached processors, then at every step one batch-1 UNet call per frame with its host alpha and one DDIM step for all
        frames.  Latents stay in their own dtype between steps; the caller's attention processors are restored."""
        unet, sched = self.unet, self.scheduler
        dev = unet.device
        state = AttnState()
        previous = get_unet_attn_processors(unet)
        set_unet_attn_processor(unet, {k: CrossFrameAttnProcessor(state, enable_interp=enable_interp) for k in previous})

        def unet1(x, t):
            return unet(x, t, return_dict=False)[0]

        def frame_by_frame(x, t):
            eps = []
            for f in range(x.shape[0]):
                state.set_alpha(weights[f])
                eps.append(unet1(x[f:f + 1], t))
            return torch.cat(eps)

        def one_pass(model, z):
            sched.set_timesteps(steps, device=dev)
            return eager_pass(model, sched, state, sched._timesteps_host, z,
                              lambda eps, t, x: sched.step(eps, t, x, eta=0.0, return_dict=False)[0])

        try:
            state.reset()
            for sid, z in ((0, latents[0:1]), (1, latents[-1:])):
                state.set_store_id(sid)
                one_pass(unet1, z)
            state.to_load()
            latents = one_pass(frame_by_frame, latents)
        finally:
            set_unet_attn_processor(unet, dict(previous))
        return latents
