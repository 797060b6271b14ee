"""Fractional-shift equivariance harness — the procedure of reference
scripts/shift_ldm_ffhq.py::shift_ldm (:49-159) on the MI355X implementation:

  1. install a CrossFrameAttnProcessor on every attention of the UNet;
  2. STORE pass: denoise the initial latent, remembering every attention's input per timestep;
  3. decode the result (the un-shifted image);
  4. for each offset tj = 1/r .. n/r latent pixels: ideal-crop shift the INITIAL latent, denoise
     it in LOAD mode (K/V from the stored maps), decode (masked), and stack
     [shifted output | bilinear-shifted un-shifted image | abs difference] vertically;
  5. restore the processors, write the frames as a GIF.

Multi-GPU: the shift offsets are independent given the STORE pass, so ranks take interleaved
offsets (each recomputes the cheap STORE pass locally) and the frames are gathered once.
Returns the frames and, per offset, the masked latent-space equivariance MSE."""
import time

import torch

from . import parallel
from .engine import DenoiseEngine, cached_engine, model_state_key
from .io_utils import image_to_tensor, save_gif_from_tensors
from .pipelines.cross_frame_attn import (AttnState, CrossFrameAttnProcessor, eager_pass, get_unet_attn_processors,
                                         set_unet_attn_processor)
from .shift_utils.metrics import mask_mse
from .shift_utils.shifters import ImageShifter
from .utils import randn_tensor


class _UnrolledEngine(DenoiseEngine):
    """DenoiseEngine whose ONE graph holds all n steps: the cross-frame processors key their stored tensors by timestep, and in
    an unrolled capture every step's slot is a fixed address - no device-side slot index, no `.item()`, no copy launches.
    `attn_state.set_timestep` gets the step's timestep as a host integer while the launches are recorded."""

    def __init__(self, unet, scheduler, batch_size, num_inference_steps, attn_state):
        super().__init__(unet, scheduler, batch_size, num_inference_steps, use_graph=True, steps_per_graph=1, branches=1)
        self.attn_state = attn_state

    def refresh_if_stale(self):
        return False            # CrossFrameSampler.run compares the model's fingerprint itself and drops every engine together

    def step(self, k=None):
        assert k in (None, self.n), "the unrolled graph runs the whole schedule"
        if self.graph is None:        # (what the warm-up step stores is overwritten by the first replay)
            self.graph, = self._capture([self.n], lambda i: self.attn_state.set_timestep(self.timesteps[i]))
        self.graph.replay()


class CrossFrameSampler:
    """The denoising passes of the shift harness (reference scripts/shift_ldm_ffhq.py:85-151: one STORE pass, then LOAD
    passes of the shifted latents) as replayed HIP graphs.  Owns the AttnState, one CrossFrameAttnProcessor (cache_kv) per
    attention and one unrolled engine per (pass kind, batch): the STORE graph writes every attention's K / V^T of every step
    into tensors of its own pool, the LOAD graphs read them in place - a new STORE replay (next seed / image) refreshes what
    the LOAD graphs see.  Cached on the pipeline: the first call captures (about the cost of two eager passes), later calls
    replay.

    interp=True (image interpolation, LDMInterpolationPipeline): the processors blend two stored passes (enable_interp); the
    STORE pass is ONE batch-2 graph of both endpoints (AttnState.PAIR: sample s fills slot s), and a LOAD engine owns a
    persistent [B] blend-weight buffer that its captured graph reads by address - run(..., alpha=...) fills it before the
    replay.  Its engines are keyed ('interp', load, batch).

    bank=True (frame sequences, LDMVideoPipeline): a STORE pass at any batch S keeps its S samples as one bank per step
    (AttnState.BANK), and a LOAD engine owns persistent [B, 2] source and [B] blend-weight buffers that its captured graph reads
    by address (each attention = one afldm_attention_bank launch) - run(..., src=..., alpha=...) fills them before the replay.
    Its engines are keyed ('bank', load, batch, S)."""

    def __init__(self, unet, scheduler, steps, interp=False, bank=False):
        """scheduler: a Schedule of `steps` evaluations, or a scheduler with .schedule(steps) (as DenoiseEngine takes)."""
        self.unet, self.scheduler, self.steps, self.interp, self.bank = unet, scheduler, steps, bool(interp), bool(bank)
        self.attn_state = AttnState()
        self.names = list(get_unet_attn_processors(unet))
        self.procs = {k: CrossFrameAttnProcessor(self.attn_state, enable_interp=self.interp, cache_kv=True, enable_bank=self.bank)
                      for k in self.names}
        self.engines = {}
        self.alphas = {}                              # interp / bank: LOAD batch -> the blend-weight buffer its graph reads
        self.sources = {}                             # bank: LOAD batch -> the [B, 2] int32 source buffer its graph reads
        self.bank_size = 0                            # bank: S of the stored pass
        self.model_key, self.stored = None, False

    def install(self):
        previous = get_unet_attn_processors(self.unet)
        set_unet_attn_processor(self.unet, dict(self.procs))
        return previous

    def run(self, latents, load, alpha=None, src=None):
        """One pass over the schedule (processors installed by the caller): STORE (load=False; attn_state is reset) or LOAD.
        interp: a STORE pass takes the two endpoints as one batch of 2; a LOAD pass needs `alpha`, one blend weight per sample.
        bank: a STORE pass takes the S sources as one batch; a LOAD pass needs `src` (per sample, its two bank slots) and `alpha`."""
        from .models.blocks import invalidate_stale_packed
        B = latents.shape[0]
        fp = model_state_key(self.unet)
        if self.model_key is None:
            # first run: record the fingerprint.  Invalidating here (as a model change) freed the packed weights that other
            # cached graphs of the same UNet - a captured ddim_inversion engine - still point at
            self.model_key = fp
        elif fp != self.model_key:                # load_state_dict / .to() / surgery since the capture: every graph is stale
            torch.cuda.synchronize()
            self.engines.clear()
            for p in self.procs.values():
                p.maps, p.kv = [dict(), dict()], [dict(), dict()]
            invalidate_stale_packed(self.unet)        # (not the copies another engine repacked for these weights)
            self.model_key, self.stored = fp, False
        if load:
            if not self.stored:
                raise RuntimeError("CrossFrameSampler: a LOAD pass needs a STORE pass first")
            self.attn_state.to_load()
            if self.interp:
                if alpha is None or len(alpha) != B:
                    raise ValueError(f"CrossFrameSampler(interp): a LOAD pass of {B} samples needs {B} blend weights")
                buf = self.alphas.get(B)
                if buf is None:
                    buf = self.alphas[B] = torch.zeros(B, dtype=torch.float32, device=self.unet.device)
                buf.copy_(torch.as_tensor(alpha, dtype=torch.float32))        # stream-ordered before the replay that reads it
                self.attn_state.set_alpha(buf)
            if self.bank:
                if alpha is None or src is None or len(alpha) != B or len(src) != B:
                    raise ValueError(f"CrossFrameSampler(bank): a LOAD pass of {B} samples needs {B} source pairs and blend weights")
                if B not in self.alphas:
                    self.alphas[B] = torch.zeros(B, dtype=torch.float32, device=self.unet.device)
                    self.sources[B] = torch.zeros(B, 2, dtype=torch.int32, device=self.unet.device)
                # stream-ordered before the replay that reads them
                self.alphas[B].copy_(torch.as_tensor(alpha, dtype=torch.float32))
                self.sources[B].copy_(torch.as_tensor(src, dtype=torch.int32).reshape(B, 2))
                self.attn_state.set_alpha(self.alphas[B])
                self.attn_state.set_sources(self.sources[B])
        else:
            self.attn_state.reset()
            if self.bank:
                self.attn_state.set_store_id(AttnState.BANK)
                self.bank_size = B
            if self.interp:
                if B != 2:
                    raise ValueError(f"CrossFrameSampler(interp): the STORE pass is one batch of the two endpoints, got {B}")
                self.attn_state.set_store_id(AttnState.PAIR)
        key = ("interp", bool(load), B) if self.interp else ("bank", bool(load), B, self.bank_size) if self.bank else (bool(load), B)
        if key not in self.engines:
            if not load:                          # a new STORE capture moves the stored tensors: the LOAD graphs read the old ones
                self.engines.clear()
            elif self.bank:                       # ONE LOAD graph: a sequence passes through it in chunks, whatever its length
                for other in [k for k in self.engines if k[1]]:
                    del self.engines[other]
            self.engines[key] = _UnrolledEngine(self.unet, self.scheduler, B, self.steps, self.attn_state)
        out = self.engines[key].run(latents)
        self.stored = self.stored or not load
        return out


def _sampler(pipeline, schedule, interp=False, bank=None):
    """The pipeline's cached CrossFrameSampler over `schedule` (a "ddim"-kind Schedule: DDIM, or the SR harness's I2SB ODE
    bridge).  interp: the interpolation sampler, cached apart; bank: the name of a banked sampler's slot (the video pipeline keeps
    two, one per schedule).  A sampler is bound to the UNet object and to the attention modules it found there, so both are
    part of its key."""
    unet = pipeline.unet
    slot = f"_xframe_bank_sampler_{bank}" if bank else "_xframe_interp_sampler" if interp else "_xframe_sampler"
    return cached_engine(pipeline, slot, schedule, None, True, unet,
                         build=lambda: CrossFrameSampler(unet, schedule, len(schedule.timesteps), interp=interp, bank=bool(bank)),
                         extra=(unet, tuple(get_unet_attn_processors(unet))))


def vae_encode(vae, x):
    return vae.encode(x).latent_dist.sample() * vae.config.scaling_factor


def vae_decode(vae, x):
    return vae.decode(x / vae.config.scaling_factor, return_dict=False)[0]


def _cross_frame_passes(pipeline, schedule, eager_steps):
    """Installs the cross-frame processors and returns (denoise, the processors to restore afterwards); denoise(latents, load)
    is one STORE (load=False) or LOAD pass.  schedule: the Schedule the passes replay as HIP graphs (the pipeline's cached
    CrossFrameSampler); None: the eager loop over the non-cached processors, where eager_steps() -> (timesteps, step_fn) sets
    the pipeline's scheduler up for one pass (step_fn(eps, t, latents) -> latents)."""
    unet = pipeline.unet
    if schedule is not None:
        sampler = _sampler(pipeline, schedule)
        return (lambda latents, load: sampler.run(latents, load).to(latents.dtype)), sampler.install()
    attn_state = AttnState()
    previous = get_unet_attn_processors(unet)
    set_unet_attn_processor(unet, {k: CrossFrameAttnProcessor(attn_state) for k in previous})

    def denoise(latents, load):
        if load:
            attn_state.to_load()
        else:
            attn_state.reset()
        timesteps, step_fn = eager_steps()
        return eager_pass(lambda x, t: unet(x, t, return_dict=False)[0], pipeline.scheduler, attn_state, timesteps,
                          latents.to(pipeline.device), step_fn)
    return denoise, previous


def _load_passes(denoise, shifted, mine, batch_offsets):
    """The LOAD passes of this rank's offsets `mine` over shifted[i] = (latent, mask): ONE batch (samples are independent; the
    cross-frame K/V of the stored pass is shared by the whole batch) or one B = 1 pass per offset.  -> {i: denoised [1, ...]}"""
    if batch_offsets and len(mine) > 1:
        den_all = denoise(torch.cat([shifted[i][0] for i in mine], 0), load=True)
        return {i: den_all[k:k + 1] for k, i in enumerate(mine)}
    return {i: denoise(shifted[i][0], load=True) for i in mine}


class _Clock:
    """Wall time per phase of a harness run ('unet_s', 'vae_s', the rest under 'other_s'), each bracketed by a device
    synchronisation; inactive (no synchronisation at all) unless the caller passes a dict to fill."""

    def __init__(self, sink):
        self.sink = sink
        if sink is not None:
            torch.cuda.synchronize()
            self.t0 = self.last = time.perf_counter()

    def lap(self, name):
        if self.sink is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.sink[name] = self.sink.get(name, 0.0) + now - self.last
            self.last = now

    def done(self):
        if self.sink is not None:
            torch.cuda.synchronize()
            self.sink["total_s"] = time.perf_counter() - self.t0


@torch.no_grad()
def shift_ldm(pipeline, num_inference_steps=50, num_shift_steps=16, output_path="results/shift_ldm.gif",
              input_path=None, generator=None, rank=0, world=1, batch_offsets=True, reference_exact=True, use_graph=True,
              timings=None):
    """batch_offsets: the LOAD passes of this rank's offsets run as ONE batch (samples are independent; the
    cross-frame K/V of the stored pass is shared by the whole batch) instead of the reference's one B = 1
    sampler run per offset (shift_ldm_ffhq.py:124-151) - 50 UNet evaluations instead of 50 per offset.

    use_graph (default): the STORE and LOAD passes run as replayed HIP graphs (CrossFrameSampler: no per-step `t.item()`
    synchronisation, no per-site clone launches, the LOAD passes attend to the stored pass's projected K / V); the graphs
    are cached on the pipeline, so the first call pays their capture and later calls (more seeds / images) replay.
    use_graph=False is the eager loop that follows reference shift_ldm_ffhq.py:85-108 statement by statement.
    timings: a dict that receives the wall time of the UNet passes ('unet_s'), the VAE calls ('vae_s'), the latent / image
    shifters ('shift_s'), the masked metrics ('metric_s'), frame assembly + device-to-host copies ('frames_s'), everything else
    ('other_s') and 'total_s' (synchronises at the phase boundaries; off when None).

    reference_exact=True (the default) follows the reference flow to the letter; reference_exact=False
    (scripts: --fixed_resize) opts into two deliberate deviations:
    * `input_path`: the image is resized to sample_size * VAE ratio (256) so that its latent has the UNet's
      sample_size; the reference resizes to (sample_size, sample_size) = 32 x 32 BEFORE the VAE
      (shift_ldm_ffhq.py:110-113), i.e. inverts a 4 x 4 latent.
    * the initial noise is drawn on the CPU (device independent) instead of on the GPU (:118-122)."""
    from .schedulers.ddim import DDIMScheduler
    from .schedulers.dpmsolver import DPMSolverMultistepScheduler
    if isinstance(pipeline.scheduler, DPMSolverMultistepScheduler):
        raise NotImplementedError("shift_ldm samples with DDIM (cross-frame STORE / LOAD passes): a pipeline whose scheduler is "
                                  "a DPMSolverMultistepScheduler is not supported")
    device = pipeline.device
    vae, unet, scheduler = pipeline.vae, pipeline.unet, pipeline.scheduler
    pipeline.set_progress_bar_config(disable=True)
    ratio = 2 ** (len(vae.up_block_types) - 1) if vae is not None else 8
    latent_shifter = ImageShifter("ideal_crop", ratio)
    image_shifter = ImageShifter()
    clock = _Clock(timings)

    def invert():
        size = unet.config.sample_size * (1 if reference_exact else ratio)
        tensor = vae_encode(vae, image_to_tensor(input_path, (size, size)).to(device))
        clock.lap("vae_s")
        scheduler.set_timesteps(num_inference_steps, device=device)
        latent = pipeline.ddim_inversion(tensor.float() if use_graph else tensor, bar=False)
        clock.lap("unet_s")
        return latent

    def eager_steps():
        scheduler.set_timesteps(num_inference_steps, device=device)
        return scheduler.timesteps, lambda eps, t, x: scheduler.step(eps, t, x, eta=0, return_dict=False)[0]

    # The reference inverts with its processors installed in their initial STORE state (shift_ldm_ffhq.py:110-116), as the eager
    # path does below; what that stores is overwritten by the STORE pass, so the graph path inverts first, on the plain
    # processors and the captured-graph loop (MyLDMPipeline.ddim_inversion, latent carried in fp32): same procedure, no side
    # effects to undo
    init_latent = invert() if use_graph and input_path is not None else None
    schedule = DDIMScheduler.from_config(scheduler.config).schedule(num_inference_steps) if use_graph else None
    denoise, previous = _cross_frame_passes(pipeline, schedule, eager_steps)
    try:
        if init_latent is None and input_path is not None:
            init_latent = invert()
        elif init_latent is None:
            # CPU-side draw (seedable, device independent) — the reference draws on the GPU
            # (shift_ldm_ffhq.py:118-122), which is not reproducible across devices
            shape = (1, unet.config.in_channels, unet.config.sample_size, unet.config.sample_size)
            if reference_exact:
                init_latent = randn_tensor(shape, device=device, generator=generator)
            else:
                init_latent = randn_tensor(shape, generator=generator).to(device)
        clock.lap("other_s")
        denoised = denoise(init_latent, load=False)
        clock.lap("unet_s")
        rec_img = vae_decode(vae, denoised) if vae is not None else None
        clock.lap("vae_s")

        offsets = torch.linspace(1 / ratio, num_shift_steps / ratio, num_shift_steps)
        mine = parallel.interleaved(num_shift_steps, rank, world)
        frames, errors = {}, {}
        shifted = {i: latent_shifter.shift(init_latent, 0, float(offsets[i])) for i in mine}
        clock.lap("shift_s")
        dens = _load_passes(denoise, shifted, mine, batch_offsets)
        clock.lap("unet_s")
        for i in mine:
            tj = float(offsets[i])
            den, mask = dens[i], shifted[i][1]
            ref_lat, _ = latent_shifter.shift(denoised, 0, tj)
            clock.lap("shift_s")
            errors[i] = float(mask_mse(den, ref_lat, mask))
            clock.lap("metric_s")
            if vae is not None:
                gt, _ = image_shifter.shift(rec_img, 0, tj * ratio)
                clock.lap("shift_s")
                img = vae_decode(vae, den * mask)
                clock.lap("vae_s")
                frames[i] = torch.cat((img, gt, torch.abs(img - gt)), -2).float().cpu()
                clock.lap("frames_s")
    finally:
        set_unet_attn_processor(unet, dict(previous))

    frames, errors = parallel.gather_indexed(world, frames, errors)
    ordered = [frames[i] for i in sorted(frames)]
    if ordered and rank == 0 and output_path:
        save_gif_from_tensors(ordered, output_path, denorm=True)
    clock.lap("other_s")
    clock.done()
    return ordered, [errors[i] for i in sorted(errors)]


def vae_encode_mode(vae, x):
    """reference scripts/shift_ldm_sr.py:31-34 (the SR harness encodes with the posterior mode)."""
    return vae.encode(x).latent_dist.mode() * vae.config.scaling_factor


@torch.no_grad()
def shift_ldm_sr(pipeline, num_inference_steps=50, num_shift_steps=16, output_path="results/shift_ldm_sr.gif",
                 input_path=None, image=None, rank=0, world=1, batch_offsets=True, use_graph=True):
    """Fractional-shift equivariance of x4 super-resolution with I2SB - the flow of reference
    scripts/shift_ldm_sr.py:43-150: degrade (bicubic x1/4, nearest x4), VAE-encode, denoise with
    cross-frame attention STORE, then for every offset shift the initial latent, denoise in LOAD mode
    and compare with the shifted reconstruction.  `image` ([1,3,H,W] in [-1,1]) replaces
    `input_path` when given; the offsets are sharded across ranks.  use_graph (default): the STORE / LOAD passes replay HIP
    graphs (CrossFrameSampler over the scheduler's ODE schedule) when the scheduler does not clip x0; otherwise - and with
    use_graph=False - the eager loop below, which follows the reference statement by statement."""
    from .af_libs.superresolution import build_sr4x
    device = pipeline.device
    vae, unet, scheduler = pipeline.vae, pipeline.unet, pipeline.scheduler
    pipeline.set_progress_bar_config(disable=True)
    ratio = 2 ** (len(vae.up_block_types) - 1)
    size = unet.config.sample_size * ratio
    sr_func = build_sr4x(device, "bicubic", size)
    latent_shifter = ImageShifter("ideal_crop", ratio)
    image_shifter = ImageShifter()

    def eager_steps():
        scheduler.set_timesteps(num_inference_steps, device=device)
        return (scheduler.timesteps[:num_inference_steps - 1],
                lambda eps, t, x: scheduler.step(eps, t, x, is_ode=True, generator=None).prev_sample)

    ode = scheduler.ode_schedule(num_inference_steps) if (use_graph and num_inference_steps >= 2) else None
    denoise, previous = _cross_frame_passes(pipeline, ode, eager_steps)
    try:
        if image is None:
            image = image_to_tensor(input_path, (size, size))
        tensor = sr_func(image.to(device).float()).clip(-1, 1)
        init_latent = vae_encode_mode(vae, tensor.to(vae.dtype)).to(unet.dtype)
        denoised = denoise(init_latent, load=False)
        rec_img = vae_decode(vae, denoised)
        offsets = torch.linspace(1 / ratio, num_shift_steps / ratio, num_shift_steps)
        frames, errors = {}, {}
        mine = parallel.interleaved(num_shift_steps, rank, world)
        shifts = {i: latent_shifter.shift(init_latent, 0, float(offsets[i])) for i in mine}
        dens = _load_passes(denoise, shifts, mine, batch_offsets)
        for i in mine:
            tj = float(offsets[i])
            (shifted, mask), den = shifts[i], dens[i]
            ref_lat, _ = latent_shifter.shift(denoised, 0, tj)
            errors[i] = float(mask_mse(den, ref_lat, mask))
            gt, _ = image_shifter.shift(rec_img, 0, tj * ratio)
            img_in = vae_decode(vae, shifted * mask)
            img = vae_decode(vae, den * mask)
            frames[i] = torch.cat((img_in, img, gt, torch.abs(img - gt)), -2).float().cpu()
    finally:
        set_unet_attn_processor(unet, dict(previous))

    frames, errors = parallel.gather_indexed(world, frames, errors)
    ordered = [frames[i] for i in sorted(frames)]
    if ordered and rank == 0 and output_path:
        save_gif_from_tensors(ordered, output_path, denorm=True)
    return ordered, [errors[i] for i in sorted(errors)]

