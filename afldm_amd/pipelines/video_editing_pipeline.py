"""LDMVideoPipeline — frame-sequence editing of reference afldm/pipelines/video_equiv_editing_pipeline.py:331-748 on the
unconditional UNet this project serves (the prompts, classifier-free guidance and the safety checker drop out):

  1. timesteps: the scheduler's, or with strength >= 0 the last int(N strength) of them (get_timesteps, :320-328);
  2. start latents, default: image2latent (:217-228, the posterior MEAN times scaling_factor) and a DDIM inversion over the
     reversed - possibly truncated - timesteps (:174-214, attn_invert=True): the anchor frame is inverted in STORE state, every
     other frame in LOAD state, attending to the anchor's maps of the same inversion timestep (:596-607);
     with use_sdedit and strength > 0: prepare_latents_sdedit (:251-318) - a posterior sample per frame, ONE randn_tensor call
     for all frames, add_noise at timesteps[0];
  3. attn_state.reset(), a STORE pass over the anchor's start latent (:648-649), a LOAD pass over ALL frames, the anchor
     included (:656-697);
  4. decode frame by frame (:719-727).

Beyond the reference: `keyframes`.  The reference has ONE anchor, frame 0; here a sorted tuple of frame indices that begins
with 0 is stored as a bank of S sources by one STORE pass at batch S, and a frame between two keyframes attends to both, blended
by its position in time (video_sources) - the interpolation pipeline's blended attention along the time axis.  keyframes=(0,)
is the reference exactly.

use_graph=True (default) keeps two banked CrossFrameSamplers on the pipeline, one over the inversion's rows and one over the
forward schedule; each holds one STORE graph at batch S and ONE LOAD graph at batch `frame_batch`, every LOAD attention being
one afldm_attention_bank launch over the cached K / V^T bank.  The frames pass in chunks of frame_batch (the last chunk
padded by repeating its last frame), the latents carried in fp32 between evaluations.  use_graph=False is the eager loop over the
non-cached processors, one frame at a time in the LOAD passes, as the reference runs them.  DESIGN.md section 25."""
import numpy as np
import torch

from ..schedulers.ddim import DDIMScheduler
from ..schedulers.schedule import Schedule
from ..utils import randn_tensor
from .cross_frame_attn import AttnState, CrossFrameAttnProcessor, get_unet_attn_processors, set_unet_attn_processor
from .ldm_pipeline import MyLDMPipeline


def check_keyframes(num_frames, keyframes):
    """`keyframes` as a tuple of ints: sorted, distinct, beginning with 0, every index below num_frames.  ValueError otherwise."""
    try:
        keys = tuple(keyframes)
    except TypeError:
        raise ValueError(f"keyframes must be a sequence of frame indices, got {keyframes!r}")
    if not keys or any(not isinstance(k, (int, np.integer)) or isinstance(k, bool) for k in keys):
        raise ValueError(f"keyframes must be a non-empty sequence of integer frame indices, got {keyframes!r}")
    keys = tuple(int(k) for k in keys)
    if keys[0] != 0:
        raise ValueError(f"keyframes must begin with frame 0 (the reference's anchor), got {keys}")
    if any(b <= a for a, b in zip(keys, keys[1:])):
        raise ValueError(f"keyframes must be sorted and distinct, got {keys}")
    if keys[-1] >= num_frames:
        raise ValueError(f"keyframe {keys[-1]} of a sequence of {num_frames} frames")
    return keys


def video_sources(num_frames, keyframes):
    """(src int32 [F, 2], alpha fp32 [F]) on the CPU: the two bank slots every frame attends to and its blend weight.  Frame f
    with k_i <= f < k_{i+1} gets (i, i + 1) and (f - k_i) / (k_{i+1} - k_i); a keyframe gets (i, i) and 0; a frame past the last
    keyframe gets (last, last) and 0."""
    keys = check_keyframes(num_frames, keyframes)
    src, alpha = [], []
    for f in range(num_frames):
        i = max(j for j, k in enumerate(keys) if k <= f)
        if f == keys[i] or i == len(keys) - 1:
            src.append((i, i))
            alpha.append(0.0)
        else:
            src.append((i, i + 1))
            alpha.append((f - keys[i]) / (keys[i + 1] - keys[i]))
    return torch.tensor(src, dtype=torch.int32).reshape(num_frames, 2), torch.tensor(alpha, dtype=torch.float32)


def video_timesteps(scheduler, num_inference_steps, strength=-1):
    """The timesteps of a call, descending, as host integers: all `num_inference_steps` of them for strength < 0, else the
    reference's get_timesteps (the last min(int(N strength), N); DDIMScheduler._sdedit_timesteps refuses a strength outside
    [0, 1] and one that leaves no step)."""
    if strength >= 0:
        return list(scheduler._sdedit_timesteps(num_inference_steps, strength))
    scheduler.set_timesteps(int(num_inference_steps))
    return list(scheduler._timesteps_host)


def inversion_rows(scheduler, timesteps):
    """(t, (mu_prev, sigma_prev, mu, sigma)) per step of the reference's ddim_inversion (:186-195) over `timesteps` (descending,
    possibly truncated) reversed: alpha_prod_t_prev = alphas_cumprod[reversed[i - 1]] for i > 0 and final_alpha_cumprod at i = 0 of
    the list as given.  latent <- mu (latent - sigma_prev eps) / mu_prev + sigma eps: afldm_ddim_step's linear form, as
    MyLDMPipeline._inversion_rows states it for the full list."""
    ts = [int(t) for t in reversed(list(timesteps))]
    ac = scheduler.alphas_cumprod
    rows = []
    for i, t in enumerate(ts):
        a_t = ac[t]
        a_prev = ac[ts[i - 1]] if i > 0 else scheduler.final_alpha_cumprod
        rows.append((t, (float(a_prev ** 0.5), float((1 - a_prev) ** 0.5), float(a_t ** 0.5), float((1 - a_t) ** 0.5))))
    return rows


class LDMVideoPipeline(MyLDMPipeline):
    """Frame-sequence editing with keyframe-banked cross-frame attention.  Build it with from_pretrained(dir) (as MyLDMPipeline)
    or from another pipeline's modules: LDMVideoPipeline(**ldm_pipeline.components)."""

    @torch.no_grad()
    def image2latent(self, image):
        """Reference :217-228: the posterior MEAN (not a sample) times scaling_factor."""
        return self.vae.encode(image.to(device=self.vae.device, dtype=self.vae.dtype)).latent_dist.mean * self.vae.config.scaling_factor

    # ------------------------------------------------------------------------------------------------ inputs
    def _frames_in(self, frames, output_type):
        """-> (tensor [F, ., ., .] on the CPU in fp32, are they latents).  Images: a list of PIL images or [F, 3, H, W] in [-1, 1]
        at the model's size; latents: [F, C, S, S] (C = the UNet's in_channels, not 3)."""
        from PIL import Image
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        if isinstance(frames, (list, tuple)) and frames and all(isinstance(f, Image.Image) for f in frames):
            if any(f.size != frames[0].size for f in frames):
                raise ValueError("LDMVideoPipeline: the frames differ in size")
            frames = torch.stack([torch.from_numpy(np.asarray(f.convert("RGB"), dtype=np.float32) / 127.5 - 1.0).permute(2, 0, 1)
                                  for f in frames])
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[0] < 1:
            raise TypeError("LDMVideoPipeline: frames is a non-empty list of PIL images or a tensor [F, 3, H, W] in [-1, 1] "
                            f"(or latents [F, {c}, {s}, {s}]), got {type(frames).__name__}"
                            + (f" {tuple(frames.shape)}" if torch.is_tensor(frames) else ""))
        x = frames.detach().float().cpu()
        if c != 3 and tuple(x.shape[1:]) == (c, s, s):
            if self.vae is None and output_type != "latent":
                raise NotImplementedError("this pipeline was built without a VAE: latent frames go with output_type='latent'")
            return x, True
        if self.vae is None:
            raise NotImplementedError(f"this pipeline was built without a VAE: pass latents [F, {c}, {s}, {s}] and "
                                      "output_type='latent'")
        r = self._vae_ratio()
        if tuple(x.shape[1:]) != (3, s * r, s * r):
            raise ValueError(f"LDMVideoPipeline: frames {tuple(x.shape)}, want [F, 3, {s * r}, {s * r}] (the model's size)")
        return x, False

    def _schedules(self, num_inference_steps, strength):
        """(forward Schedule, inversion Schedule) of a call.  The forward rows are DDIMScheduler.step's for the kept timesteps
        (their prev_t is t - T // N whatever the truncation); the inversion rows are inversion_rows over the same list."""
        sch = self.scheduler
        ts = video_timesteps(sch, num_inference_steps, strength)
        n_all = int(num_inference_steps)
        sch.set_timesteps(n_all)
        fwd = Schedule.of(sch, "ddim", ts, sch.coefficients, _video_steps=n_all, _video_kept=len(ts))
        rows = inversion_rows(sch, ts)
        inv = Schedule.of(sch, "ddim", [t for t, _ in rows], [c for _, c in rows], _video_inversion_steps=n_all,
                          _video_inversion_kept=len(ts))
        return fwd, inv

    # ------------------------------------------------------------------------------------------------ the call
    @torch.no_grad()
    def __call__(self, frames, num_inference_steps=50, strength=-1, use_sdedit=False, keyframes=(0,), generator=None,
                 frame_batch=16, output_type="pil", return_dict=True, use_graph=True):
        """frames: a list of PIL images or [F, 3, H, W] in [-1, 1] at the model's size (or latents [F, C, S, S] with
        output_type='latent': the VAE is then not needed).  strength < 0: the whole schedule; strength in (0, 1]: its last
        int(N strength) steps.  use_sdedit (with strength > 0): start from the noised frames instead of their inversion; the
        draws come from `generator`.  keyframes: see the module docstring.  frame_batch: the batch of the ONE LOAD graph
        (use_graph).  Returns the edited frames (output_type 'latent' / 'pt' / 'np' / 'pil', as MyLDMPipeline); the UNet's
        attention processors are as they were on return, also after an exception.  No trained weights exist here: nothing is
        claimed about sample quality or temporal consistency."""
        self._refuse_dpm("LDMVideoPipeline")
        if not isinstance(self.scheduler, DDIMScheduler):
            raise NotImplementedError(f"LDMVideoPipeline samples with DDIM (inversion + cross-frame STORE / LOAD passes): a "
                                      f"pipeline whose scheduler is a {type(self.scheduler).__name__} is not supported")
        if not isinstance(frame_batch, (int, np.integer)) or isinstance(frame_batch, bool) or frame_batch < 1:
            raise ValueError(f"LDMVideoPipeline: frame_batch must be an integer >= 1, got {frame_batch!r}")
        x, is_latent = self._frames_in(frames, output_type)
        F_ = x.shape[0]
        keys = check_keyframes(F_, keyframes)
        src, alpha = video_sources(F_, keys)
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        fwd, inv = self._schedules(num_inference_steps, strength)
        dev, unet = self.unet.device, self.unet
        if dev.type != "cuda":
            raise RuntimeError("LDMVideoPipeline needs the UNet on an MI355X ('cuda') device; there is no CPU path")
        run = self._graph_passes if use_graph else self._eager_passes
        if use_sdedit and strength > 0:
            start = self._sdedit_start(x, is_latent, fwd.timesteps[0], generator)
        else:
            lat = x.to(dev) if is_latent else torch.cat([self.image2latent(x[f:f + 1]) for f in range(F_)])
            start = run("inv", inv, lat, keys, src, alpha, int(frame_batch), all_frames=False)
        out = run("fwd", fwd, start, keys, src, alpha, int(frame_batch), all_frames=True).to(unet.dtype)
        if output_type == "latent":
            return out
        scale = self.vae.config.scaling_factor
        decoded = torch.cat([self.vae.decode(out[f:f + 1].to(self.vae.dtype) / scale).sample for f in range(F_)])
        return self._images(decoded, output_type, return_dict)

    def _sdedit_start(self, x, is_latent, t0, generator):
        """Reference prepare_latents_sdedit (:251-318): per frame the posterior sample times scaling_factor (latents as they
        are), ONE randn_tensor call for all frames in the UNet's dtype, add_noise at the first kept timestep."""
        dev, dtype = self.unet.device, self.unet.dtype
        if is_latent:
            init = x.to(dev)
        else:
            init = torch.cat([self.vae.encode(x[f:f + 1].to(device=self.vae.device, dtype=self.vae.dtype)).latent_dist.sample(generator)
                              for f in range(x.shape[0])]) * self.vae.config.scaling_factor
        noise = randn_tensor(tuple(init.shape), generator=generator, device=dev, dtype=dtype)
        ab = float(self.scheduler.alphas_cumprod[int(t0)])
        return (ab ** 0.5) * init.float() + ((1 - ab) ** 0.5) * noise.float()

    # ------------------------------------------------------------------------------------------------ graph path
    def _graph_passes(self, which, schedule, latents, keys, src, alpha, frame_batch, all_frames):
        """One STORE pass over the keyframes' latents at batch S, then LOAD passes in chunks of frame_batch over all frames
        (the forward schedule) or over the frames that are no keyframes (the inversion: the STORE pass is the keyframes' own
        inversion).  Returns fp32 [F, C, S, S]."""
        from ..harness import _sampler
        smp = _sampler(self, schedule, bank=which)
        previous = smp.install()
        try:
            x = latents.to(device=self.unet.device, dtype=torch.float32)
            out = x.clone()
            stored = smp.run(x[list(keys)].contiguous(), load=False)
            todo = list(range(x.shape[0])) if all_frames else [f for f in range(x.shape[0]) if f not in keys]
            if not all_frames:
                out[list(keys)] = stored
            for c0 in range(0, len(todo), frame_batch):
                real = todo[c0:c0 + frame_batch]
                idx = real + [real[-1]] * (frame_batch - len(real))            # padding: the chunk's last frame again
                got = smp.run(x[idx].contiguous(), load=True, src=src[idx], alpha=alpha[idx])
                out[real] = got[:len(real)]
            return out
        finally:
            set_unet_attn_processor(self.unet, dict(previous))

    # ------------------------------------------------------------------------------------------------ eager path
    def _eager_passes(self, which, schedule, latents, keys, src, alpha, frame_batch, all_frames):
        """The same passes as the reference runs them: the non-cached banked processors, one batch-S STORE pass, then one
        batch-1 LOAD pass per frame with its host source pair and alpha.  Latents stay in the UNet's dtype between steps."""
        from .. import ops
        unet, dev = self.unet, self.unet.device
        state = AttnState()
        previous = get_unet_attn_processors(unet)
        set_unet_attn_processor(unet, {k: CrossFrameAttnProcessor(state, enable_bank=True) for k in previous})

        def one_pass(z):
            for t, coef in zip(schedule.timesteps, schedule.rows):
                state.set_timestep(t)
                eps = unet(z, t, return_dict=False)[0]
                z = ops.ddim_step_flat(z.float().contiguous(), eps.float().contiguous(), coef).to(z.dtype)
            return z

        try:
            x = latents.to(device=dev, dtype=unet.dtype)
            out = x.clone()
            state.reset()
            state.set_store_id(AttnState.BANK)
            stored = one_pass(x[list(keys)].contiguous())
            if not all_frames:
                out[list(keys)] = stored
            state.to_load()
            for f in (range(x.shape[0]) if all_frames else [f for f in range(x.shape[0]) if f not in keys]):
                state.set_sources(src[f:f + 1].to(dev))
                state.set_alpha(float(alpha[f]))
                out[f:f + 1] = one_pass(x[f:f + 1])
            return out.float()
        finally:
            set_unet_attn_processor(unet, dict(previous))
