"""MyLDMPipeline — surface of reference afldm/pipelines/ldm_pipeline.py:17-160 on MI355X.

`__call__(output_type='latent')` is the throughput entry point: the DDIM loop runs as a
replayed HIP graph (afldm_amd.engine.DenoiseEngine); other output types decode through the
(alias-free) AutoencoderKL of afldm_amd.models.vae."""
import inspect
import json
import os
from dataclasses import replace

import torch

from ..engine import cached_engine
from ..models.unet_2d import UNet2DModel
from ..schedulers.ddim import DDIMScheduler
from ..schedulers.dpmsolver import DPMSolverMultistepScheduler
from ..schedulers.schedule import KINDS, Schedule
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
            # (not through _sample, on purpose: _sample shows the engine the re-created scheduler, and this engine's .scheduler
            # stays the Schedule it was built from, which tests/test_sde_host.py relies on)
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

    @torch.no_grad()
    def sample_mixed(self, num_inference_steps, generator=None, latents=None, output_type="pil", return_dict=True, slots=None,
                     steps_per_graph=5, engines=1, eta=None, seeds=None):
        """One sample per entry of `num_inference_steps`, each with its own step count, in request order - DDIM (eta = 0), or
        DPM-Solver(++) when `self.scheduler` is a DPMSolverMultistepScheduler (as __call__ chooses) - through a
        SamplingServer (afldm_amd/serving.py): the requests share the batch-`slots` graphs (default: one slot per request, 64 at
        the most, per engine) and a slot that finishes takes the next request.  generator: None, one torch.Generator (the start
        latents are drawn from it request by request) or one per request; latents: the start latents [n, C, S, S] instead.
        Request i is pipe(batch_size=1, num_inference_steps=num_inference_steps[i], generator=generator[i]) to the rounding of
        the convolutions at another batch size.  output_type as __call__.  The server is kept for the next call with the same
        scheduler class: one built for DDIM takes no DPM requests, so swapping the scheduler builds another.
        eta, seeds: a float (or one per request) and one integer seed per request - request i with eta != 0 is a stochastic DDIM
        sample whose noise is a function of seeds[i] (SamplingServer.submit(eta=, seed=)); the server then also takes "seeded"
        schedules.  With seeds and neither generator nor latents, request i starts from manual_seed(seeds[i])."""
        from ..serving import SamplingServer
        counts = [int(n) for n in num_inference_steps]
        etas = [0.0] * len(counts) if eta is None else [float(v) for v in eta] if isinstance(eta, (list, tuple)) else [float(eta)] * len(counts)
        if len(etas) != len(counts) or (seeds is not None and len(seeds) != len(counts)):
            raise ValueError(f"sample_mixed: {len(etas)} eta values and {None if seeds is None else len(seeds)} seeds for "
                             f"{len(counts)} requests")
        if isinstance(generator, (list, tuple)) and len(generator) != len(counts):
            raise ValueError(f"sample_mixed: {len(generator)} generators for {len(counts)} requests")
        if latents is not None and latents.shape[0] != len(counts):
            raise ValueError(f"sample_mixed: {latents.shape[0]} start latents for {len(counts)} requests")
        slots = max(1, min(len(counts), 64)) if slots is None else int(slots)
        kinds = SamplingServer.default_kinds(self) + (("seeded",) if any(etas) or seeds is not None else ())
        key = (id(self.unet), slots, int(steps_per_graph), int(engines), kinds)
        if key not in self.__dict__.get("_slot_servers", ()):
            self.__dict__["_slot_servers"] = {key: SamplingServer(self, slots, steps_per_graph, engines, kinds=kinds)}
        server = self.__dict__["_slot_servers"][key]
        tickets = [server.submit(n, generator[i] if isinstance(generator, (list, tuple)) else generator,
                                 None if latents is None else latents[i:i + 1], eta=etas[i],
                                 seed=None if seeds is None else seeds[i]) for i, n in enumerate(counts)]
        server.run()
        if not tickets:
            raise ValueError("sample_mixed: no requests")
        return server.decode(tickets, output_type, return_dict)

    # ------------------------------------------------------------------------------------------------ seeded stochastic sampling
    @torch.no_grad()
    def sample_seeded_latents(self, seeds, eta=1.0, num_inference_steps=50, latents=None, use_graph=True):
        """Stochastic DDIM, one sample per entry of `seeds` (integers in [0, 2^63)), with counter-based device noise: the noise
        of sample i at step k is a function of (seeds[i], k, element) that the update kernel computes in registers
        (include/afldm_hip_noise.h) - no noise buffer and no host draw, and the sample does not depend on its batch position or
        its neighbours.  The start latents of sample i are randn_tensor(generator=manual_seed(seeds[i])) unless `latents`
        [n, C, S, S] is given.  use_graph: SeededEngine on replayed HIP graphs; otherwise the eager loop - afldm_counter_noise
        materialises the step's noise and afldm_sde_step applies it, which differs from the graph path by float rounding only.
        eta = 0 is the plain "ddim" schedule: pipe(generator=[manual_seed(s) for s in seeds]) exactly.  A DPM scheduler raises.
        Returns fp32 latents.  The stream is this project's own: it does not match torch's generators."""
        from .. import ops
        from ..engine import SeededEngine, check_seeds
        self._refuse_dpm("sample_seeded_latents")
        host = check_seeds(seeds, len(seeds), "sample_seeded_latents")
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        shape = (len(seeds), c, s, s)
        if latents is None:
            latents = randn_tensor(shape, generator=[torch.Generator().manual_seed(int(v)) for v in host.tolist()])
        elif tuple(latents.shape) != shape:
            raise ValueError(f"sample_seeded_latents: latents {tuple(latents.shape)}, want {shape}")
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        if float(eta) == 0.0:
            eng = cached_engine(self, "_engines", self.scheduler.schedule(num_inference_steps), shape[0], use_graph, self.unet)
            eng.scheduler = self.scheduler
            return eng.run(latents)
        sched = self.scheduler.seeded_schedule(num_inference_steps, eta)
        if use_graph:
            eng = cached_engine(self, "_seeded_engines", sched, shape[0], True, self.unet, SeededEngine)
            eng.scheduler = self.scheduler
            return eng.run(latents, known=host)
        dev = self.unet.device
        if dev.type != "cuda":
            raise RuntimeError("sample_seeded_latents needs the UNet on an MI355X ('cuda') device; there is no CPU path")
        x = (latents.to(device=dev, dtype=torch.float32) * sched.init_noise_sigma).contiguous()
        seeds_dev, rows = host.to(dev), sched.table(dev)
        first = torch.zeros(1, dtype=torch.int32, device=dev)          # (every launch gets its step's row alone)
        for k, t in enumerate(self.progress_bar(list(sched.timesteps))):
            eps = self.unet.forward_nhwc(ops.to_nhwc(x, self.unet.dtype), t)
            z = ops.counter_noise(seeds_dev, torch.full((shape[0],), k, dtype=torch.int32, device=dev), shape)
            x = ops.sde_step(x, eps, z.unsqueeze(0), rows[k].contiguous(), first)
        return x

    @torch.no_grad()
    def sample_seeded(self, seeds, eta=1.0, num_inference_steps=50, latents=None, use_graph=True, output_type="pil",
                      return_dict=True):
        """Sample images with seeded stochastic DDIM: sample_seeded_latents, then decode.  output_type as __call__; 'latent'
        returns the latents in the UNet's dtype."""
        out = self.sample_seeded_latents(seeds, eta, num_inference_steps, latents, use_graph)
        return self._deliver(out.to(self.unet.dtype), output_type, return_dict)

    # ------------------------------------------------------------------------------------------------ parallel-in-time sampling
    @torch.no_grad()
    def sample_parallel_latents(self, batch_size=1, num_inference_steps=50, window=8, tolerance=0.1, generator=None, latents=None,
                                use_graph=True, eta=0.0):
        """Parallel-in-time DDIM sampling (ParaDiGMS, Shih et al., NeurIPS 2023; diffusers' DDIMParallelScheduler pipeline, whose
        default `tolerance` this takes): `window` consecutive steps of every image are evaluated as one UNet batch of batch_size x
        window rows and iterated to their fixed point - Picard iteration on the sampler's recurrence.  One iteration evaluates
        eps at the window's current estimates, sweeps the DDIM update along the window with those outputs, accepts every state
        up to the first whose estimate moved by more than tolerance^2 in mean square (at least one: the first state of a window
        is always exact) and slides the window that far.  An image therefore costs `iterations` evaluations of batch `window`
        instead of num_inference_steps evaluations of batch 1, and iterations <= num_inference_steps always.  tolerance = 0
        accepts a state only when its predecessors did not move at all: the plain DDIM sampler, one state per iteration;
        window = 1 is that sampler too.  tolerance > 0 trades accuracy for iterations.  How many iterations a trained model
        takes at a given tolerance has not been measured here, and no claim about sample quality is made for any tolerance.

        The start latents are drawn as __call__ draws them.  use_graph: PicardEngine on replayed HIP graphs (afldm_picard_sweep /
        _stride / _slide behind the UNet); otherwise the statement-by-statement loop below: per-row timesteps into the UNet, the
        recurrence and the errors in torch, the stride decided on the host.  Only the deterministic DDIM sampler has this form:
        eta != 0 and a DPM scheduler raise NotImplementedError.  Needs no VAE.  Returns (fp32 latents [B, C, S, S], stats) with
        stats = {"iterations", "evaluations" (iterations x batch_size x window), "strides" (per iteration, one per image)}."""
        from ..engine import PicardEngine
        self._refuse_dpm("sample_parallel_latents")
        if not isinstance(self.scheduler, DDIMScheduler):
            raise NotImplementedError(f"sample_parallel_latents needs a DDIMScheduler: it is not implemented with "
                                      f"{type(self.scheduler).__name__} (PicardEngine takes any 'ddim' Schedule directly)")
        if eta != 0.0:
            raise NotImplementedError("sample_parallel_latents: eta != 0 (a stochastic schedule) needs a pre-drawn noise row per "
                                      "state of the window, which is not implemented")
        window, tolerance = PicardEngine.check_window(window, tolerance)
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        if latents is None:
            latents = randn_tensor((batch_size, c, s, s), generator=generator)
        if latents.dim() != 4 or tuple(latents.shape[1:]) != (c, s, s):
            raise ValueError(f"sample_parallel_latents: latents {tuple(latents.shape)}, want [B, {c}, {s}, {s}]")
        sched = self.scheduler.schedule(num_inference_steps)
        if use_graph:
            eng = cached_engine(self, "_picard_engines", sched, latents.shape[0], True, self.unet, PicardEngine, window=window,
                                tolerance=tolerance)
            eng.scheduler = self.scheduler
            return eng.run(latents), eng.stats
        return self._picard_loop(sched, latents, window, tolerance)

    def _picard_loop(self, sched, latents, window, tolerance):
        """sample_parallel_latents(use_graph=False): the four steps of an iteration as torch statements."""
        if self.unet.device.type != "cuda":
            raise RuntimeError("sample_parallel_latents needs the UNet on an MI355X ('cuda') device; there is no CPU path")
        dev, n, Wn, P = self.unet.device, len(sched.rows), window, latents.shape[0]
        rows, ts = sched.table(dev), sched.timesteps
        x = (latents.to(device=dev, dtype=torch.float32) * sched.init_noise_sigma).unsqueeze(0).repeat(Wn + 1, 1, 1, 1, 1)
        base, strides = [0] * P, []
        while min(base) < n:
            if len(strides) >= n:
                raise RuntimeError(f"sample_parallel_latents: {len(strides)} iterations of a {n}-row schedule, cursors at {base}")
            # 1. evaluate: row j P + p at X[j] of image p with its own timestep (a row past the end: evaluated, not used)
            t = torch.tensor([float(ts[min(base[p] + j, n - 1)]) for j in range(Wn) for p in range(P)], device=dev)
            eps = self.unet(x[:Wn].reshape((Wn * P,) + tuple(x.shape[2:])).to(self.unet.dtype), t).sample.float().reshape(x[:Wn].shape)
            # 2. sweep
            y = [x[0]]
            for j in range(Wn):
                on = torch.tensor([base[p] + j < n for p in range(P)], device=dev).reshape(P, 1, 1, 1)
                c0, c1, c2, c3 = (rows[[min(base[p] + j, n - 1) for p in range(P)], k].reshape(P, 1, 1, 1) for k in range(4))
                y.append(torch.where(on, c2 * ((y[j] - c1 * eps[j]) / c0) + c3 * eps[j], y[j]))
            y = torch.stack(y)
            err = (y[1:] - x[1:]).pow(2).mean(dim=(2, 3, 4)).tolist()          # [Wn][P]
            # 3. stride, 4. slide
            took = []
            for p in range(P):
                if base[p] >= n:
                    took.append(0)
                    continue
                over = [j + 1 for j in range(Wn) if base[p] + j < n and err[j][p] > tolerance ** 2]
                sp = min(min(over + [Wn]), n - base[p])
                x[:, p] = y[[min(j + sp, Wn) for j in range(Wn + 1)], p]
                base[p] += sp
                took.append(sp)
            strides.append(took)
        stats = {"iterations": len(strides), "evaluations": len(strides) * P * Wn, "strides": strides}
        return x[0].clone(), stats

    @torch.no_grad()
    def sample_parallel(self, batch_size=1, num_inference_steps=50, window=8, tolerance=0.1, generator=None, latents=None,
                        use_graph=True, eta=0.0, output_type="pil", return_dict=True):
        """Sample images with parallel-in-time DDIM sampling: sample_parallel_latents, then decode.  output_type as __call__;
        'latent' returns the latents in the UNet's dtype.  The statistics of the run stay in `pipe.parallel_stats`."""
        out, self.__dict__["parallel_stats"] = self.sample_parallel_latents(batch_size, num_inference_steps, window, tolerance,
                                                                            generator, latents, use_graph, eta)
        return self._deliver(out.to(self.unet.dtype), output_type, return_dict)

    def _deliver(self, latents, output_type, return_dict):
        """'latent' -> the latents; 'pt' -> decoded tensor in [-1, 1]; 'np' / 'pil' -> [0, 1] NHWC arrays / PIL images
        (wrapped in ImagePipelineOutput unless return_dict is False)."""
        if output_type == "latent":
            return latents
        if self.vae is None:
            raise NotImplementedError("this pipeline was built without a VAE: use output_type='latent'")
        return self._images(self._decode(latents), output_type, return_dict)

    def _decode(self, latents):
        """The VAE's decoding of scaled latents, in [-1, 1] and the VAE's dtype (_deliver; SamplingServer.decode)."""
        return self.vae.decode(latents.to(self.vae.dtype) / self.vae.config.scaling_factor).sample

    def _images(self, decoded, output_type, return_dict):
        """A decoded tensor in [-1, 1] as `output_type` 'pt', 'np' or 'pil' (_deliver)."""
        if output_type == "pt":
            return decoded
        arrays = (decoded / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()
        images = self.numpy_to_pil(arrays) if output_type == "pil" else arrays
        return ImagePipelineOutput(images=images) if return_dict else (images,)

    def _sample(self, sched, shape, generator, latents, use_graph, slot, eager, cls=None, batch=None, known=None, **kw):
        """The protocol every sampler on a Schedule shares.  The draws come from `generator` through sched.drawer(shape): the start
        latents first (unless `latents` is given; on the CPU for CPU generators, else on the device: the per-evaluation draws'
        rule), then per evaluation the slots sched.slots(k) in slot order.  use_graph: the engine cached in `slot` - cls (default
        DenoiseEngine) with its own keyword arguments kw, at `batch` (default shape[0]) - runs them, with the static per-run
        tensors `known`.  Otherwise the eager loop: the latents scaled by init_noise_sigma and carried in fp32 like the engine,
        x <- eager(x, t, row, zs) per evaluation, zs the kind's slots as fp32 device tensors, None where not drawn.  Returns fp32."""
        dev = self.unet.device
        draw = sched.drawer(generator, shape, dev, self.unet.dtype)
        if latents is None:
            latents = draw()
        if use_graph:
            eng = cached_engine(self, slot, sched, shape[0] if batch is None else batch, True, self.unet, cls, **kw)
            eng.scheduler = self.scheduler
            return eng.run(latents, draw=draw, **({} if known is None else {"known": known}))
        x = (latents.to(device=dev, dtype=torch.float32) * sched.init_noise_sigma).contiguous()
        for k, (t, row) in enumerate(self.progress_bar(list(zip(sched.timesteps, sched.rows)))):
            on = sched.slots(k)
            zs = [draw().to(device=dev, dtype=torch.float32).contiguous() if j in on else None for j in range(KINDS[sched.kind][1])]
            x = eager(x, t, row, zs)
        return x

    def _vae_ratio(self):
        """Pixels per latent along an axis."""
        return getattr(self.vae, "downsample_ratio", None) or 2 ** (len(self.vae.config.block_out_channels) - 1)

    def _encode_mode(self, image):
        """image in [-1, 1] -> the posterior mode times scaling_factor."""
        from ..harness import vae_encode_mode
        return vae_encode_mode(self.vae, image.to(device=self.unet.device, dtype=self.vae.dtype))

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

    # ------------------------------------------------------------------------------------------------ RePaint inpainting
    def _refuse_dpm(self, what):
        if isinstance(self.scheduler, DPMSolverMultistepScheduler):
            raise NotImplementedError(f"{what} needs a DDIMScheduler: it is not implemented with {type(self.scheduler).__name__}")

    @torch.no_grad()
    def inpaint_latents(self, known_latents, latent_mask, num_inference_steps=50, eta=0.0, jump_length=10, jump_n_sample=10,
                        generator=None, latents=None, use_graph=True):
        """RePaint (Lugmayr et al., CVPR 2022, Algorithm 1; diffusers RePaintPipeline) in latent space: sample latents that agree
        with `known_latents` [B, C, S, S] where `latent_mask` [B | 1, 1, S, S] is 1 and are generated where it is 0 (soft values
        blend).  Needs no VAE.  The schedule is DDIMScheduler.repaint_schedule: every UNet evaluation ends in one
        afldm_repaint_step, on replayed HIP graphs (use_graph) or in the eager loop below, which makes the same draws from
        `generator` in the same order - the start latents (unless `latents` is given), then per evaluation z_k, z_u, z_b where
        the schedule draws them - and carries the latents in fp32 like the engine.  Returns latents in the UNet's dtype; with
        a hard mask the kept latents are `known_latents` exactly (to that dtype)."""
        from .. import ops
        self._refuse_dpm("inpaint_latents")
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        if known_latents.dim() != 4 or tuple(known_latents.shape[1:]) != (c, s, s):
            raise ValueError(f"inpaint_latents: known_latents {tuple(known_latents.shape)}, want [B, {c}, {s}, {s}]")
        B = known_latents.shape[0]
        if latent_mask.dim() != 4 or tuple(latent_mask.shape[1:]) != (1, s, s) or latent_mask.shape[0] not in (1, B):
            raise ValueError(f"inpaint_latents: latent_mask {tuple(latent_mask.shape)}, want [{B} or 1, 1, {s}, {s}]")
        if latents is not None and tuple(latents.shape) != (B, c, s, s):
            raise ValueError(f"inpaint_latents: latents {tuple(latents.shape)}, want {(B, c, s, s)}")
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.repaint_schedule(num_inference_steps, eta, jump_length, jump_n_sample)
        dev = self.unet.device
        known = known_latents.to(device=dev, dtype=torch.float32).contiguous()
        mask = latent_mask.to(device=dev, dtype=torch.float32)
        full = None if use_graph else mask.expand(B, c, s, s).contiguous()

        def eager(x, t, row, zs):
            eps = self.unet(x.to(self.unet.dtype), t).sample
            return ops.repaint_step_flat(x, eps.float().contiguous(), known, full, zs, row)
        return self._sample(sched, (B, c, s, s), generator, latents, use_graph, "_repaint_engines", eager,
                            known=(known, mask)).to(self.unet.dtype)

    @torch.no_grad()
    def inpaint(self, image, mask, num_inference_steps=50, eta=0.0, jump_length=10, jump_n_sample=10, generator=None, latents=None,
                use_graph=True, mask_mode="min", composite=True, output_type="pil", return_dict=True):
        """Inpaint `image` [B, 3, H, W] in [-1, 1] where `mask` [B | 1, 1, H, W] is 0 and keep it where the mask is 1.  The image is
        encoded with the posterior mode times scaling_factor (harness.vae_encode_mode), the mask pooled to the latent grid over
        the VAE's down-sampling blocks (afldm_mask_pool; mask_mode 'min': a latent is kept only if every pixel under it is,
        'mean': the kept fraction as a soft mask), the latents sampled by inpaint_latents and decoded.  composite: the result is
        m image + (1 - m) decoded in pixel space, in fp32, so that kept pixels are the input's exactly.  output_type as
        __call__; 'latent' returns the sampled latents."""
        image, mask, known, latent_mask = self._inpaint_inputs(image, mask, mask_mode)
        out = self.inpaint_latents(known, latent_mask, num_inference_steps, eta, jump_length, jump_n_sample, generator, latents,
                                   use_graph)
        if output_type == "latent":
            return out
        decoded = self.vae.decode(out.to(self.vae.dtype) / self.vae.config.scaling_factor).sample
        if composite:
            decoded = self._inpaint_composite(decoded, image, mask)
        return self._images(decoded, output_type, return_dict)

    def _inpaint_inputs(self, image, mask, mask_mode="min", who="inpaint"):
        """What `inpaint` samples from (and SamplingServer.submit_inpaint): (image, mask) as fp32 on the device, the image's
        latents and the mask pooled to the latent grid.  Raises what `inpaint` raises."""
        from .. import ops
        self._refuse_dpm(who)
        if self.vae is None:
            raise NotImplementedError(f"this pipeline was built without a VAE: use {who}_latents")
        if mask_mode not in ("min", "mean"):
            raise ValueError(f"{who}: mask_mode {mask_mode!r} (want 'min' or 'mean')")
        r = self._vae_ratio()
        s = self.unet.config.sample_size
        if image.dim() != 4 or tuple(image.shape[1:]) != (3, s * r, s * r):
            raise ValueError(f"{who}: image {tuple(image.shape)}, want [B, 3, {s * r}, {s * r}]")
        if mask.dim() != 4 or tuple(mask.shape[1:]) != (1, s * r, s * r) or mask.shape[0] not in (1, image.shape[0]):
            raise ValueError(f"{who}: mask {tuple(mask.shape)}, want [{image.shape[0]} or 1, 1, {s * r}, {s * r}]")
        dev = self.unet.device
        image = image.to(device=dev, dtype=torch.float32)
        mask = mask.to(device=dev, dtype=torch.float32).contiguous()
        known = self._encode_mode(image)
        latent_mask = ops.mask_pool(mask, r, ops.MASK_MIN if mask_mode == "min" else ops.MASK_MEAN)
        return image, mask, known, latent_mask

    @staticmethod
    def _inpaint_composite(decoded, image, mask):
        """m image + (1 - m) decoded in pixel space, in fp32: kept pixels are the input's exactly."""
        return mask * image + (1 - mask) * decoded.float()

    # ------------------------------------------------------------------------------------------------ image-to-image (SDEdit)
    @torch.no_grad()
    def img2img_latents(self, orig_latents, strength=0.6, change_map=None, num_inference_steps=50, eta=0.0, generator=None,
                        noise=None, use_graph=True):
        """Image-to-image sampling in latent space: SDEdit (Meng et al., ICLR 2022; the reference's get_timesteps and
        prepare_latents_sdedit, video_equiv_editing_pipeline.py:251-328) with a per-element change map (Differential Diffusion,
        Levin & Fried 2023).  `orig_latents` [B, C, S, S] is noised to the first of the last n = int(num_inference_steps * strength)
        timesteps and denoised from there.  `change_map` [B | 1, 1, S, S] in [0, 1] gives every element a strength of its own:
        1 is regenerated from the first evaluation, 0 is never touched and comes back exactly, and a value between is held on the
        original's noised trajectory until the schedule's threshold (n - 1 - k) / n falls below it; None: all ones, plain SDEdit.
        Needs no VAE.  The schedule is DDIMScheduler.sdedit_schedule: every UNet evaluation ends in one afldm_sdedit_step, on
        replayed HIP graphs (use_graph) or in the eager loop below, which makes the same draws from `generator` in the same
        order - the run's one noise z in the model's dtype (unless `noise` is given), then per evaluation z_u where the schedule
        draws it - and carries the latents in fp32 like the engine.  Returns latents in the UNet's dtype."""
        from .. import ops
        from ..engine import SDEditEngine
        self._refuse_dpm("img2img_latents")
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        if orig_latents.dim() != 4 or tuple(orig_latents.shape[1:]) != (c, s, s):
            raise ValueError(f"img2img_latents: orig_latents {tuple(orig_latents.shape)}, want [B, {c}, {s}, {s}]")
        B = orig_latents.shape[0]
        if change_map is not None and (change_map.dim() != 4 or tuple(change_map.shape[1:]) != (1, s, s)
                                       or change_map.shape[0] not in (1, B)):
            raise ValueError(f"img2img_latents: change_map {tuple(change_map.shape)}, want [{B} or 1, 1, {s}, {s}]")
        if noise is not None and tuple(noise.shape) != (B, c, s, s):
            raise ValueError(f"img2img_latents: noise {tuple(noise.shape)}, want {(B, c, s, s)}")
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.sdedit_schedule(num_inference_steps, strength, eta)
        k0s, k1s = self.scheduler.sdedit_start(num_inference_steps, strength)
        dev = self.unet.device
        shape = (B, c, s, s)
        orig = orig_latents.to(device=dev, dtype=torch.float32).contiguous()
        cmap = (torch.ones(1, 1, s, s, device=dev) if change_map is None else change_map).to(device=dev, dtype=torch.float32)
        if noise is None:
            noise = sched.drawer(generator, shape, dev, self.unet.dtype)()
        z = noise.to(device=dev, dtype=torch.float32).contiguous()
        # the start, by the formula every held element follows: the row (p = q = 0, no clip, a = b = c = 0, k0_start, k1_start,
        # thr = +inf) holds everything at k0_start orig + k1_start z
        zero = torch.zeros_like(orig)
        start = ops.sdedit_step_flat(zero, zero, orig, zero, z, None,
                                     (0.0, 0.0, -float("inf"), float("inf"), 0.0, 0.0, 0.0, k0s, k1s, float("inf")))
        full = None if use_graph else cmap.expand(B, c, s, s).contiguous()

        def eager(x, t, row, zs):
            eps = self.unet(x.to(self.unet.dtype), t).sample
            return ops.sdedit_step_flat(x, eps.float().contiguous(), orig, full, z, zs[0], row)
        return self._sample(sched, shape, generator, start, use_graph, "_sdedit_engines", eager, cls=SDEditEngine,
                            known=(orig, cmap, z)).to(self.unet.dtype)

    @torch.no_grad()
    def img2img(self, image, strength=0.6, change_map=None, num_inference_steps=50, eta=0.0, generator=None, noise=None,
                use_graph=True, composite=True, output_type="pil", return_dict=True):
        """Change `image` [B, 3, H, W] in [-1, 1] by `strength`; `change_map` [B | 1, 1, H, W] in [0, 1] says per pixel how much
        (0 = keep, 1 = regenerate; None: everywhere).  The image is encoded with the posterior mode times scaling_factor
        (harness.vae_encode_mode), the map pooled to the latent grid by its mean over the VAE's down-sampling blocks
        (afldm_mask_pool), the latents sampled by img2img_latents and decoded.  composite: pixels whose change value is exactly 0
        are the input's, in fp32; nothing is blended elsewhere.  output_type as __call__; 'latent' returns the sampled latents."""
        image, change_map, orig, latent_map = self._img2img_inputs(image, strength, change_map)
        out = self.img2img_latents(orig, strength, latent_map, num_inference_steps, eta, generator, noise, use_graph)
        if output_type == "latent":
            return out
        decoded = self.vae.decode(out.to(self.vae.dtype) / self.vae.config.scaling_factor).sample
        if composite and change_map is not None:
            decoded = self._img2img_composite(decoded, image, change_map)
        return self._images(decoded, output_type, return_dict)

    def _img2img_inputs(self, image, strength, change_map, who="img2img"):
        """What `img2img` samples from (and SamplingServer.submit_img2img): (image, change_map) as fp32 on the device (the map may
        be None), the image's latents and the map pooled to the latent grid (None for None).  Raises what `img2img` raises."""
        from .. import ops
        self._refuse_dpm(who)
        if self.vae is None:
            raise NotImplementedError(f"this pipeline was built without a VAE: use {who}_latents")
        r = self._vae_ratio()
        s = self.unet.config.sample_size
        if image.dim() != 4 or tuple(image.shape[1:]) != (3, s * r, s * r):
            raise ValueError(f"{who}: image {tuple(image.shape)}, want [B, 3, {s * r}, {s * r}]")
        if change_map is not None and (change_map.dim() != 4 or tuple(change_map.shape[1:]) != (1, s * r, s * r)
                                       or change_map.shape[0] not in (1, image.shape[0])):
            raise ValueError(f"{who}: change_map {tuple(change_map.shape)}, want [{image.shape[0]} or 1, 1, {s * r}, {s * r}]")
        if not 0.0 <= float(strength) <= 1.0:
            raise ValueError(f"{who}: strength = {strength} must be in [0, 1]")
        dev = self.unet.device
        image = image.to(device=dev, dtype=torch.float32)
        latent_map = None
        if change_map is not None:
            change_map = change_map.to(device=dev, dtype=torch.float32).contiguous()
            latent_map = ops.mask_pool(change_map, r, ops.MASK_MEAN)
        return image, change_map, self._encode_mode(image), latent_map

    @staticmethod
    def _img2img_composite(decoded, image, change_map):
        """Pixels whose change value is exactly 0 are the input's, in fp32; nothing is blended elsewhere."""
        return torch.where(change_map == 0, image, decoded.float())

    # ------------------------------------------------------------------------------------------------ bit-reversible sampling
    @staticmethod
    def _rev_is_code(what, code):
        from ..reversible import ReversibleCode
        if not isinstance(code, ReversibleCode):
            raise TypeError(f"{what}: code must be a ReversibleCode, got {type(code).__name__}")

    def _rev_code_check(self, what, code, k, num_inference_steps, exact):
        """A ReversibleCode against the call that takes it: the level it sits at always; with `exact` also everything its bits
        depend on."""
        from .. import _lib
        from ..engine import model_state_key
        self._rev_is_code(what, code)
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        if code.hi.dim() != 4 or tuple(code.hi.shape[1:]) != (c, s, s) or code.lo.shape != code.hi.shape:
            raise ValueError(f"{what}: a code of {tuple(code.hi.shape)} / {tuple(code.lo.shape)}, want [B, {c}, {s}, {s}] twice")
        if code.k != k:
            raise ValueError(f"{what}: the code sits at level {code.k}, and this call starts from level {k}")
        if not exact:
            return
        diff = code.mismatches(batch=code.hi.shape[0], dtype=self.unet.dtype, model_key=model_state_key(self.unet),
                               library=_lib.library_hash(), num_inference_steps=int(num_inference_steps))
        if diff:
            raise ValueError(f"{what}: the code was made with " + ", ".join(f"{n} = {a!r} (now {b!r})" for n, a, b in diff) +
                             ": the steps would not be undone bit for bit.  exact=False runs it anyway, with no such guarantee")

    def _rev_run(self, sched, start, use_graph):
        """A "rev" schedule from `start` (latents or a ReversibleCode) to a ReversibleCode: ReversibleEngine on replayed graphs, or
        the eager loop over ops.rev_step_flat, which carries the same int64 pair."""
        from .. import _lib, ops
        from ..engine import ReversibleEngine, model_state_key
        from ..reversible import ReversibleCode, decode
        cfg = sched.config
        sampling, from_code = cfg["_rev_direction"] == "sample", cfg["_rev_from_code"]
        B = (start.hi if from_code else start).shape[0]
        if use_graph:
            slot = f"_rev_{cfg['_rev_direction']}_{'code' if from_code else 'start'}_engines"
            eng = cached_engine(self, slot, sched, B, True, self.unet, ReversibleEngine)
            eng.scheduler = self.scheduler
            return eng.run(start)
        dev = self.unet.device
        if dev.type != "cuda":
            raise RuntimeError("the reversible sampler needs the UNet on an MI355X ('cuda') device; there is no CPU path")
        bad = torch.zeros(B, dtype=torch.int32, device=dev)
        if from_code:
            far, near = ((start.hi, start.lo) if sampling else (start.lo, start.hi))
            far, near = far.to(dev).clone(), near.to(dev).clone()
        else:
            near = ops.rev_encode((start.to(device=dev, dtype=torch.float32) * sched.init_noise_sigma).contiguous(), bad)
            far = near.clone()
        x = decode(near)
        for t, row in self.progress_bar(list(zip(sched.timesteps, sched.rows))):
            eps = self.unet(x.to(self.unet.dtype), t).sample
            x = ops.rev_step_flat(far, near, eps.float().contiguous(), bad, row)
        rows = bad.nonzero().flatten().tolist()
        if rows:
            raise FloatingPointError(f"the reversible sampler met non-finite values or int64 overflow in the latents of batch rows "
                                     f"{rows}: the states of these rows are INVALID")
        levels = len(sched.timesteps) + (1 if from_code else 0)
        hi, lo = (far, near) if sampling else (near, far)
        return ReversibleCode(hi, lo, 1 if sampling else levels, cfg["_rev_steps"], None, B, self.unet.dtype,
                              model_state_key(self.unet), _lib.library_hash())

    @torch.no_grad()
    def sample_reversible_latents(self, batch_size=1, num_inference_steps=50, generator=None, latents=None, code=None,
                                  use_graph=True, return_code=False, exact=True):
        """Sample with the bit-reversible sampler: a two-step (leapfrog) form of deterministic DDIM, after BDIA (Zhang et al., ECCV
        2024) at gamma = 1, with the latents carried as int64 fixed point on the grid 2^-32 (DDIMScheduler.reversible_schedule,
        afldm_rev_step).  It costs one UNet evaluation per step like DDIM and is NOT the DDIM sampler: its samples differ, and no
        claim about their quality is made.  What it gives is algebraic: invert_reversible(code=...) of the returned code walks the
        same integers back and returns the start noise's integers exactly, and sampling from a code invert_reversible returned
        gives back the inverted latents' integers exactly.

        From noise - `latents`, or drawn as __call__ draws them - N evaluations; from `code` = the (X_N, X_N-1) invert_reversible
        returned, N - 1 (its strength, if any, applies).  The guarantee holds when the code's batch size, model dtype, weights,
        library build and step count are the call's: a code that differs raises ValueError, and exact=False runs it anyway
        WITHOUT any bit guarantee.  use_graph: ReversibleEngine on replayed HIP graphs; otherwise the eager loop over
        afldm_rev_step_flat, which carries the same int64 pair.  Only deterministic epsilon-prediction DDIM has this form.
        Returns the fp32 latents, with return_code (latents, ReversibleCode at level 1)."""
        self._refuse_dpm("sample_reversible_latents")
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        if code is not None:
            if latents is not None:
                raise ValueError("sample_reversible_latents: give latents or a code, not both")
            self._rev_is_code("sample_reversible_latents", code)
            levels = len(self.scheduler.reversible_levels(num_inference_steps, code.strength)[0]) - 1
            self._rev_code_check("sample_reversible_latents", code, levels, num_inference_steps, exact)
            sched, start = self.scheduler.reversible_schedule(num_inference_steps, "sample", True, code.strength), code
        else:
            sched = self.scheduler.reversible_schedule(num_inference_steps, "sample", False)
            if latents is None:
                latents = sched.drawer(generator, (batch_size, c, s, s), self.unet.device, self.unet.dtype)()
            if latents.dim() != 4 or tuple(latents.shape[1:]) != (c, s, s):
                raise ValueError(f"sample_reversible_latents: latents {tuple(latents.shape)}, want [B, {c}, {s}, {s}]")
            start = latents
        out = self._rev_run(sched, start, use_graph)
        if code is not None:
            out = replace(out, strength=code.strength)
        return (out.latents(), out) if return_code else out.latents()

    @torch.no_grad()
    def sample_reversible(self, batch_size=1, num_inference_steps=50, generator=None, latents=None, code=None, output_type="pil",
                          return_dict=True, use_graph=True, return_code=False, exact=True):
        """Sample images with the bit-reversible sampler: sample_reversible_latents, then decode.  output_type as __call__;
        'latent' returns the latents in the UNet's dtype.  With return_code: (that, the ReversibleCode at level 1, whose
        .latents() are the unrounded fp32 latents)."""
        lat, out = self.sample_reversible_latents(batch_size, num_inference_steps, generator, latents, code, use_graph, True, exact)
        got = self._deliver(lat.to(self.unet.dtype), output_type, return_dict)
        return (got, out) if return_code else got

    @torch.no_grad()
    def invert_reversible(self, image_or_latents=None, code=None, num_inference_steps=50, strength=None, use_graph=True, exact=True):
        """Invert with the bit-reversible sampler (sample_reversible_latents): returns the ReversibleCode (X_N, X_N-1) at the noise
        end, from which sample_reversible(code=...) returns to where this started, integer for integer.

        From `code` = the (X_1, X_0) a sampling run returned: N - 1 evaluations, and the result's `hi` is the integers of the noise
        that run started from.  From an image [B, 3, H, W] in [-1, 1] (encoded with the posterior mode times scaling_factor) or
        latents [B, C, S, S]: N evaluations, the first of them a plain DDIM inversion step from level 0 to level 1 with eps
        evaluated at the image (the reference's inversion starts the same way).  The true eps at level 0 is unknowable, so what
        comes back is a code - a noise-like pair that samples back to the image exactly - not "the" noise that made the image.
        strength: invert up the first int(N strength) levels only, as img2img counts them.  exact as sample_reversible_latents."""
        self._refuse_dpm("invert_reversible")
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        if (code is None) == (image_or_latents is None):
            raise ValueError("invert_reversible: give an image (or latents) or a code, and not both")
        if code is not None:
            self._rev_code_check("invert_reversible", code, 1, num_inference_steps, exact)
            sched, start = self.scheduler.reversible_schedule(num_inference_steps, "invert", True, strength), code
        else:
            x = image_or_latents
            if x.dim() != 4:
                raise ValueError(f"invert_reversible: {tuple(x.shape)}, want an image [B, 3, H, W] or latents [B, {c}, {s}, {s}]")
            if tuple(x.shape[1:]) != (c, s, s):
                if self.vae is None:
                    raise NotImplementedError("this pipeline was built without a VAE: give invert_reversible latents "
                                              f"[B, {c}, {s}, {s}]")
                r = self._vae_ratio()
                if tuple(x.shape[1:]) != (3, s * r, s * r):
                    raise ValueError(f"invert_reversible: image {tuple(x.shape)}, want [B, 3, {s * r}, {s * r}]")
                x = self._encode_mode(x)
            sched, start = self.scheduler.reversible_schedule(num_inference_steps, "invert", False, strength), x
        return replace(self._rev_run(sched, start, use_graph), strength=strength)

    # ------------------------------------------------------------------------------------------------ ILVR reference guidance
    @torch.no_grad()
    def ilvr_latents(self, ref_latents, down_factor=4, range_t=0, num_inference_steps=50, eta=1.0, phi=None, generator=None,
                     latents=None, use_graph=True):
        """ILVR (Choi et al., ICCV 2021, Algorithm 1) in latent space: sample latents that share the low-frequency content of
        `ref_latents` [B, C, S, S].  After every reverse step down to timestep `range_t` the low band phi(x') of the proposal is
        replaced by that of the reference noised to the same level.  phi is the ideal low-pass LPF_RFFT(cutoff = 1 /
        down_factor) as its [S, S] circulant L, phi(x) = L x L^T: an exact projection that commutes with every circular shift,
        so the guidance is alias-free like the model (at S = 32 the factors 2, 4, 8 keep 15, 7, 3 frequencies per axis).  `phi`:
        an [S, S] matrix used for both axes instead.  Needs no VAE.  The schedule is DDIMScheduler.ilvr_schedule: every UNet
        evaluation ends in one afldm_ilvr_step, on replayed HIP graphs (use_graph) or in the eager loop below, which makes the
        same draws from `generator` in the same order - the start latents (unless `latents` is given), then per evaluation z_k,
        z_u where the schedule draws them - and carries the latents in fp32 like the engine.  Returns latents in the UNet's dtype."""
        from .. import ops
        from ..af_libs.ideal_lpf import ilvr_filter
        self._refuse_dpm("ilvr_latents")
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        if ref_latents.dim() != 4 or tuple(ref_latents.shape[1:]) != (c, s, s):
            raise ValueError(f"ilvr_latents: ref_latents {tuple(ref_latents.shape)}, want [B, {c}, {s}, {s}]")
        B = ref_latents.shape[0]
        if latents is not None and tuple(latents.shape) != (B, c, s, s):
            raise ValueError(f"ilvr_latents: latents {tuple(latents.shape)}, want {(B, c, s, s)}")
        if phi is not None and tuple(phi.shape) != (s, s):
            raise ValueError(f"ilvr_latents: phi {tuple(phi.shape)}, want {(s, s)}")
        dev = self.unet.device
        L = (phi if phi is not None else ilvr_filter(s, down_factor)).to(device=dev, dtype=torch.float32).contiguous()
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.ilvr_schedule(num_inference_steps, eta, range_t)
        ref = ref_latents.to(device=dev, dtype=torch.float32).contiguous()

        def eager(x, t, row, zs):
            eps = self.unet(x.to(self.unet.dtype), t).sample
            return ops.ilvr_step_flat(x, eps.float().contiguous(), ref, zs, L, L, row)
        return self._sample(sched, (B, c, s, s), generator, latents, use_graph, "_ilvr_engines", eager,
                            known=(ref, L)).to(self.unet.dtype)

    @torch.no_grad()
    def ilvr(self, image, down_factor=4, range_t=0, num_inference_steps=50, eta=1.0, phi=None, generator=None, latents=None,
             use_graph=True, output_type="pil", return_dict=True):
        """Sample images that share the coarse content of `image` [B, 3, H, W] in [-1, 1]: the image is encoded with the
        posterior mode times scaling_factor (as inpaint), the latents sampled by ilvr_latents and decoded.  output_type as
        __call__; 'latent' returns the sampled latents."""
        self._refuse_dpm("ilvr")
        if self.vae is None:
            raise NotImplementedError("this pipeline was built without a VAE: use ilvr_latents")
        r = self._vae_ratio()
        s = self.unet.config.sample_size
        if image.dim() != 4 or tuple(image.shape[1:]) != (3, s * r, s * r):
            raise ValueError(f"ilvr: image {tuple(image.shape)}, want [B, 3, {s * r}, {s * r}]")
        out = self.ilvr_latents(self._encode_mode(image), down_factor, range_t, num_inference_steps, eta, phi, generator, latents, use_graph)
        return self._deliver(out, output_type, return_dict)

    # ------------------------------------------------------------------------------------------------ perturbed-attention guidance
    def pag_sites(self, pag_applied_layers):
        """The attention modules `pag_applied_layers` names, as a sorted tuple of module paths.  A name is a key of
        get_unet_attn_processors without its '.processor', or a prefix of one that ends on a '.' boundary: 'mid_block',
        'up_blocks.1' and 'up_blocks.1.attentions.0' are all valid.  A name that matches nothing raises ValueError."""
        from .cross_frame_attn import get_unet_attn_processors
        if isinstance(pag_applied_layers, str):
            pag_applied_layers = (pag_applied_layers,)
        keys = [k[:-len(".processor")] for k in get_unet_attn_processors(self.unet)]
        sites = set()
        for name in pag_applied_layers:
            hit = [k for k in keys if k == name or k.startswith(str(name) + ".")]
            if not hit:
                raise ValueError(f"pag_applied_layers: {name!r} matches no attention block (there are: {', '.join(keys)})")
            sites.update(hit)
        return tuple(sorted(sites))

    @torch.no_grad()
    def pag_latents(self, batch_size=1, pag_scale=3.0, pag_applied_layers=("mid_block",), guidance_rescale=0.0, eta=0.0,
                    num_inference_steps=50, generator=None, latents=None, use_graph=True):
        """Perturbed-attention guidance (Ahn et al. 2024; diffusers PAGMixin) in latent space: the guidance that needs no condition.
        Every evaluation runs the UNet and, in the same batch, the UNet whose self-attention map at `pag_applied_layers`
        (pag_sites) is the identity, e and e_p, and steps with g = e + pag_scale (e - e_p); `guidance_rescale` in [0, 1] pulls
        the standard deviation of g back towards e's per sample (diffusers rescale_noise_cfg).  The schedule is
        DDIMScheduler.pag_schedule: every evaluation ends in one afldm_pag_step on replayed HIP graphs (use_graph, PAGEngine) or
        in the eager loop below over afldm_pag_step_flat, which makes the same draws from `generator` in the same order - the
        start latents (unless `latents` is given), then with eta != 0 one tensor per evaluation - and carries the latents in
        fp32 like the engine.  pag_scale = 0 is allowed and still evaluates both halves.  Needs no VAE.  Returns latents in
        the UNet's dtype.  The UNet's attention processors are as they were on return, also after an exception."""
        from .. import ops
        from ..engine import PAGEngine, pag_processors
        self._refuse_dpm("pag_latents")
        sites = self.pag_sites(pag_applied_layers)
        if not sites and float(pag_scale) > 0.0:
            raise ValueError("pag_latents: pag_scale > 0 needs at least one attention block in pag_applied_layers")
        c, s, dev = self.unet.config.in_channels, self.unet.config.sample_size, self.unet.device
        B = int(batch_size) if latents is None else latents.shape[0]
        shape = (B, c, s, s)
        if latents is not None and tuple(latents.shape) != shape:
            raise ValueError(f"pag_latents: latents {tuple(latents.shape)}, want [B, {c}, {s}, {s}]")
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.pag_schedule(num_inference_steps, eta, pag_scale, guidance_rescale)

        def eager(x, t, row, zs):
            with pag_processors(self.unet, sites):
                eps2 = self.unet(torch.cat([x, x]).to(self.unet.dtype), t).sample.float()
            return ops.pag_step_flat(x, eps2[:B].contiguous(), eps2[B:].contiguous(), zs[0], row)
        return self._sample(sched, shape, generator, latents, use_graph, "_pag_engines", eager, PAGEngine,
                            sites=sites).to(self.unet.dtype)

    @torch.no_grad()
    def pag(self, batch_size=1, pag_scale=3.0, pag_applied_layers=("mid_block",), guidance_rescale=0.0, eta=0.0,
            num_inference_steps=50, generator=None, latents=None, use_graph=True, output_type="pil", return_dict=True):
        """Sample images with perturbed-attention guidance: pag_latents, then decode.  output_type as __call__; 'latent' returns
        the sampled latents."""
        self._refuse_dpm("pag")
        out = self.pag_latents(batch_size, pag_scale, pag_applied_layers, guidance_rescale, eta, num_inference_steps, generator,
                               latents, use_graph)
        return self._deliver(out, output_type, return_dict)

    # ------------------------------------------------------------------------------------------------ classifier-free guidance
    def _cfg_rows(self, class_labels, null_label, null_embedding, guided):
        """(labels for unet.forward on the evaluated batch, the class rows [R, D] CFGEngine takes, B): the conditional rows, and
        behind them - when guided - the unconditional rows: the row of `null_label` (default num_class_embeds - 1) of an
        nn.Embedding table, `null_embedding` [D] or [B, D] (default zeros) of an 'identity' class embedding."""
        unet = self.unet
        if getattr(unet, "class_embedding", None) is None:
            raise ValueError("classifier-free guidance needs a class-conditional UNet (num_class_embeds, or class_embed_type='identity')")
        cond = unet.class_embed(class_labels)
        B, D = cond.shape
        if B == 0:
            raise ValueError("cfg_latents: no class labels")
        table = hasattr(unet.class_embedding, "num_embeddings")
        if table and null_embedding is not None:
            raise ValueError("null_embedding goes with class_embed_type='identity'; an embedding table takes null_label")
        if not table and null_label is not None:
            raise ValueError("null_label goes with an embedding table (num_class_embeds); class_embed_type='identity' takes null_embedding")
        labels = torch.as_tensor(class_labels)
        if not guided:
            return (labels.reshape(-1) if table else labels), cond, B
        if table:
            null = unet.class_embedding.num_embeddings - 1 if null_label is None else int(null_label)
            both = torch.cat([labels.reshape(-1).to("cpu", torch.int64), torch.full((B,), null, dtype=torch.int64)])
            return both, unet.class_embed(both), B
        null = torch.zeros(B, D) if null_embedding is None else torch.as_tensor(null_embedding).float().cpu()
        if null.dim() == 1:
            null = null.unsqueeze(0).expand(B, -1)
        if tuple(null.shape) != (B, D):
            raise ValueError(f"null_embedding {tuple(null.shape)}, want [{D}] or [{B}, {D}]")
        both = torch.cat([labels.float().cpu(), null])
        return both, unet.class_embed(both), B

    @torch.no_grad()
    def cfg_latents(self, class_labels, guidance_scale=3.0, guidance_rescale=0.0, null_label=None, null_embedding=None, eta=0.0,
                    num_inference_steps=50, generator=None, latents=None, use_graph=True):
        """Class-conditional sampling with classifier-free guidance (Ho & Salimans 2022) in latent space, one sample per entry of
        `class_labels` - integer labels [B] for a UNet with an embedding table (num_class_embeds), float rows [B, temb_dim] for
        class_embed_type 'identity'.  Every evaluation runs the UNet on 2 B rows, the B conditional ones and behind them the B
        unconditional ones, e_c and e_u, and steps with g = e_c + (guidance_scale - 1) (e_c - e_u) - diffusers'
        e_u + guidance_scale (e_c - e_u) in another order, so not bit-identical to it; `guidance_rescale` in [0, 1] pulls the
        standard deviation of g back towards e_c's per sample (diffusers rescale_noise_cfg).  The unconditional rows: with an
        embedding table the row of `null_label`, default num_class_embeds - 1 - the convention of training with the LAST class
        as the dropped-label ("null") class; a checkpoint trained otherwise must say which row it is - and with 'identity'
        `null_embedding`, default zeros.  guidance_scale = 1 evaluates the B conditional rows only and applies the scheduler's own
        update.  The schedule is DDIMScheduler.cfg_schedule: replayed HIP graphs (use_graph, CFGEngine: the class rows are data,
        other labels replay the same graphs) or the eager loop below over unet.forward and afldm_pag_step_flat, which makes the
        same draws from `generator` in the same order - the start latents (unless `latents` is given), then with eta != 0 one
        tensor per evaluation - and carries the latents in fp32 like the engine.  Needs no VAE.  Returns latents in the UNet's
        dtype."""
        from .. import ops
        from ..engine import CFGEngine
        self._refuse_dpm("classifier-free guidance")
        w = float(guidance_scale)
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.cfg_schedule(num_inference_steps, eta, w, guidance_rescale)      # (also checks the two settings)
        guided = w != 1.0
        if not guided:
            sched = (self.scheduler.stochastic_schedule(num_inference_steps, eta) if float(eta) != 0.0
                     else self.scheduler.schedule(num_inference_steps))
        labels, rows, B = self._cfg_rows(class_labels, null_label, null_embedding, guided)
        c, s = self.unet.config.in_channels, self.unet.config.sample_size
        shape = (B, c, s, s)
        if latents is not None and tuple(latents.shape) != shape:
            raise ValueError(f"cfg_latents: latents {tuple(latents.shape)}, want [{B}, {c}, {s}, {s}] for {B} class labels")

        def eager(x, t, row, zs):
            if guided:
                eps2 = self.unet(torch.cat([x, x]).to(self.unet.dtype), t, labels).sample.float()
                return ops.pag_step_flat(x, eps2[:B].contiguous(), eps2[B:].contiguous(), zs[0], row)
            e = self.unet(x.to(self.unet.dtype), t, labels).sample.float().contiguous()
            if sched.kind == "ddim":
                return ops.ddim_step_flat(x, e, row)
            return ops.pag_step_flat(x, e, e, zs[0], row + (0.0, 0.0, 0.0, 0.0))        # the "sde" row: s = 0, phi = 0
        return self._sample(sched, shape, generator, latents, use_graph, "_cfg_engines", eager, CFGEngine, known=rows,
                            guided=guided).to(self.unet.dtype)

    @torch.no_grad()
    def cfg(self, class_labels, guidance_scale=3.0, guidance_rescale=0.0, null_label=None, null_embedding=None, eta=0.0,
            num_inference_steps=50, generator=None, latents=None, use_graph=True, output_type="pil", return_dict=True):
        """Sample images of the classes `class_labels` with classifier-free guidance: cfg_latents, then decode.  output_type as
        __call__; 'latent' returns the sampled latents."""
        self._refuse_dpm("classifier-free guidance")
        out = self.cfg_latents(class_labels, guidance_scale, guidance_rescale, null_label, null_embedding, eta, num_inference_steps,
                               generator, latents, use_graph)
        return self._deliver(out, output_type, return_dict)

    # ------------------------------------------------------------------------------------------------ self-attention guidance
    def sag_site_of(self, sag_site):
        """The ONE attention module `sag_site` names, as a module path: a key of get_unet_attn_processors without its
        '.processor', or a prefix of one on a '.' boundary (as pag_sites resolves names) that selects exactly one module -
        'mid_block' and 'up_blocks.1.attentions.0' are valid, 'up_blocks.1' is not where that block has several attentions.
        Anything else raises ValueError listing the candidates."""
        from .cross_frame_attn import get_unet_attn_processors
        keys = [k[:-len(".processor")] for k in get_unet_attn_processors(self.unet)]
        hit = [k for k in keys if k == sag_site or k.startswith(str(sag_site) + ".")] if isinstance(sag_site, str) else []
        if len(hit) != 1:
            raise ValueError(f"sag_site: {sag_site!r} names {len(hit)} attention blocks, want exactly one of: {', '.join(keys)}")
        return hit[0]

    @torch.no_grad()
    def sag_latents(self, batch_size=1, sag_scale=0.75, sag_site="mid_block", blur_kernel_size=9, blur_sigma=1.0,
                    blur_boundary="reflect", guidance_rescale=0.0, eta=0.0, num_inference_steps=50, generator=None,
                    latents=None, use_graph=True, masks=None, return_masks=False):
        """Self-attention guidance (Hong et al., ICCV 2023; diffusers StableDiffusionSAGPipeline restricted to an unconditional
        UNet) in latent space.  Every step evaluates the UNet, e = UNet(x, t), while the attention block `sag_site` (sag_site_of)
        also reports the attention mass each of its keys receives (afldm_attn_key_mass; heads-mean, summed over the queries);
        where that mass exceeds 1 the predicted x0 = p x + q e is Gaussian-blurred (`blur_kernel_size` taps, `blur_sigma`;
        `blur_boundary` 'reflect' as diffusers pads, or 'circular', under which the degradation commutes with circular integer
        shifts) and re-noised with e itself, x_d = x + M (G x0 - x0) / p (afldm_sag_degrade); e_d = UNet(x_d, t) with the
        processors as found; and the step is pag_latents' with g = e + sag_scale (e - e_d) (`guidance_rescale` likewise).  The two
        evaluations are dependent, so a step costs two UNet launches of batch B.

        `sag_site` defaults to diffusers' "mid_block", which on the FFHQ model is the 2 x 2 level: a map of only 4 tokens, each
        covering a quarter of the latent plane.  scripts/sag_ffhq.py picks the 8 x 8 up-block attention instead.

        The schedule is DDIMScheduler.sag_schedule: replayed HIP graphs (use_graph, SAGEngine) or the eager loop below over
        afldm_sag_degrade_flat and afldm_pag_step_flat, which makes the same draws from `generator` in the same order as pag_latents
        - the start latents (unless `latents` is given), then with eta != 0 one tensor per step - and carries the latents in fp32
        like the engine.  Eager loop only: return_masks=True returns (latents, masses) with the fp32 [B, T] masses of every
        step, and masks= replays a list of [B, T] boolean masks, one per step, instead of thresholding (with use_graph=True it
        raises ValueError).  sag_scale = 0 is allowed and still runs both evaluations.  Needs no VAE.  Returns latents in the
        UNet's dtype.  The UNet's attention processors are as they were on return, also after an exception."""
        from .. import ops
        from ..engine import SAGEngine, sag_processor
        self._refuse_dpm("sag_latents")
        site = self.sag_site_of(sag_site)
        taps = ops.gaussian_taps(blur_kernel_size, blur_sigma)
        if blur_boundary not in ("reflect", "circular"):
            raise ValueError(f"sag_latents: blur_boundary {blur_boundary!r} (want 'reflect' or 'circular')")
        if use_graph and (masks is not None or return_masks):
            raise ValueError("sag_latents: masks= and return_masks=True belong to the eager loop (use_graph=False)")
        c, s, dev = self.unet.config.in_channels, self.unet.config.sample_size, self.unet.device
        B = int(batch_size) if latents is None else latents.shape[0]
        shape = (B, c, s, s)
        if latents is not None and tuple(latents.shape) != shape:
            raise ValueError(f"sag_latents: latents {tuple(latents.shape)}, want [B, {c}, {s}, {s}]")
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.sag_schedule(num_inference_steps, eta, sag_scale, guidance_rescale)
        if masks is not None and len(masks) != len(sched.timesteps):
            raise ValueError(f"sag_latents: {len(masks)} masks for {len(sched.timesteps)} steps")
        pq = sched.table("cpu")[:, :2].tolist()         # (p, q) as the engine's kernel reads them: rounded once to fp32
        masses, steps = [], iter(range(len(sched.timesteps)))

        def eager(x, t, row, zs):
            k = next(steps)
            with sag_processor(self.unet, site) as proc:
                e = self.unet(x.to(self.unet.dtype), t).sample.float().contiguous()
            mass = proc.mass
            masses.append(mass)
            if masks is not None:
                m = masks[k]
                if tuple(m.shape) != tuple(mass.shape) or m.dtype != torch.bool:
                    raise ValueError(f"sag_latents: masks[{k}] is {m.dtype} {tuple(m.shape)}, want bool {tuple(mass.shape)}")
                mass = m.to(dev).float() * 2.0          # 2 > 1: masked; 0: not
            x_d = ops.sag_degrade_flat(x, e, mass.contiguous(), taps, blur_boundary, *pq[k])
            e_d = self.unet(x_d.to(self.unet.dtype), t).sample.float().contiguous()
            return ops.pag_step_flat(x, e, e_d, zs[0], row)
        out = self._sample(sched, shape, generator, latents, use_graph, "_sag_engines", eager, SAGEngine, site=site, taps=taps,
                           boundary=blur_boundary).to(self.unet.dtype)
        return (out, masses) if return_masks else out

    @torch.no_grad()
    def sag(self, batch_size=1, sag_scale=0.75, sag_site="mid_block", blur_kernel_size=9, blur_sigma=1.0, blur_boundary="reflect",
            guidance_rescale=0.0, eta=0.0, num_inference_steps=50, generator=None, latents=None, use_graph=True, masks=None,
            return_masks=False, output_type="pil", return_dict=True):
        """Sample images with self-attention guidance: sag_latents, then decode.  output_type as __call__; 'latent' returns the
        sampled latents.  With return_masks=True (eager loop) the result is (images, masses)."""
        self._refuse_dpm("sag")
        out = self.sag_latents(batch_size, sag_scale, sag_site, blur_kernel_size, blur_sigma, blur_boundary, guidance_rescale, eta,
                               num_inference_steps, generator, latents, use_graph, masks, return_masks)
        if return_masks:
            return self._deliver(out[0], output_type, return_dict), out[1]
        return self._deliver(out, output_type, return_dict)

    # ------------------------------------------------------------------------------------------------ MultiDiffusion panoramas
    def panorama_geometry(self, height, width, stride=None, circular=False):
        """The panorama.Geometry of a height x width canvas (latent units) under this UNet's window: `stride` (default
        sample_size // 4) on both axes, the x axis circular on request."""
        from ..panorama import Geometry
        s = self.unet.config.sample_size
        stride = s // 4 if stride is None else int(stride)
        return Geometry.grid(height, width, s, stride, stride, circular_x=circular)

    @torch.no_grad()
    def panorama_latents(self, height, width, stride=None, circular=False, eta=0.0, num_inference_steps=50, batch_size=1,
                         generator=None, latents=None, use_graph=True):
        """MultiDiffusion (Bar-Tal et al., ICML 2023; diffusers StableDiffusionPanoramaPipeline) in latent space: sample `batch_size`
        canvases of height x width latents, larger than the sample_size^2 window the UNet was trained on.  Every evaluation runs
        the UNet on the overlapping windows of the canvas (panorama.window_origins with `stride`, default sample_size // 4;
        `circular` wraps the x axis, for a seamless 360-degree strip) as ONE batch of batch_size * nwin planes, takes the DDIM
        reverse step (eta: its stochastic form) in every window and replaces each canvas element by the plain mean of the steps of
        the windows that cover it.  That fusion assumes that windows offset by a fraction of a window agree where they overlap -
        the shift-equivariance an alias-free model has.  The schedule is DDIMScheduler.panorama_schedule: every evaluation ends
        in one afldm_pano_step, on replayed HIP graphs (use_graph), or runs statement by statement in the eager loop below, which
        makes the same draws from `generator` in the same order - the start canvas (unless `latents` [P, C, height, width] is
        given), then one canvas-shaped tensor in the model's dtype per evaluation whose sigma is not 0.  Needs no VAE.  Returns
        the fp32 canvas [P, C, height, width]."""
        from .. import ops
        from ..engine import PanoramaEngine
        self._refuse_dpm("panorama_latents")
        geom = self.panorama_geometry(height, width, stride, circular)
        c, s, dev = self.unet.config.in_channels, self.unet.config.sample_size, self.unet.device
        P = int(batch_size) if latents is None else latents.shape[0]
        shape = (P, c, geom.Hc, geom.Wc)
        if latents is not None and tuple(latents.shape) != shape:
            raise ValueError(f"panorama_latents: latents {tuple(latents.shape)}, want [P, {c}, {geom.Hc}, {geom.Wc}]")
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.panorama_schedule(num_inference_steps, eta)
        ones = torch.ones(s, s, dtype=torch.float32, device=dev)

        def eager(x, t, row, zs):
            p, q, lo, hi, a, b, d, cz = row
            win = ops.window_crop(x, geom)                                    # [P * nwin, C, S, S]
            eps = self.unet(win.to(self.unet.dtype), t).sample.float()
            x0 = torch.clamp(p * win + q * eps, lo, hi)                       # every window's own prediction of the clean latents
            x = a * x + b * ops.window_fuse(x0.contiguous(), ones, geom) + d * ops.window_fuse(eps.contiguous(), ones, geom)
            if zs[0] is not None:
                x = x + cz * zs[0]
            return x.contiguous()
        return self._sample(sched, shape, generator, latents, use_graph, "_pano_engines", eager, PanoramaEngine, P * geom.nwin,
                            geometry=geom)

    @torch.no_grad()
    def decode_panorama(self, canvas, geometry):
        """canvas [P, C, Hc, Wc] latents -> fp32 [P, 3, r Hc, r Wc] in [-1, 1]: the canvas is decoded window by window, at the
        origins it was sampled with (one AF-VAE decode of batch nwin per canvas), and the decodes are blended by afldm_window_fuse
        under the separable triangular feather t[i] = min(i + 1, n - i), n = r S.  This is a blend of INDEPENDENT window decodes,
        not a decode of the whole canvas: the AF-VAE's filters and normalisations are global per plane, so a plane of another
        size is another function, and the decoder only exists at the window's size."""
        from .. import ops
        from ..panorama import feather
        if self.vae is None:
            raise NotImplementedError("this pipeline was built without a VAE: use panorama_latents")
        r = self._vae_ratio()
        dev, n = self.unet.device, geometry.nwin
        win = ops.window_crop(canvas.to(device=dev, dtype=torch.float32).contiguous(), geometry)
        scale = self.vae.config.scaling_factor
        dec = torch.cat([self.vae.decode(win[i:i + n].to(self.vae.dtype) / scale).sample for i in range(0, win.shape[0], n)])
        t = torch.tensor(feather(geometry.S * r), dtype=torch.float32, device=dev)
        return ops.window_fuse(dec.contiguous(), torch.outer(t, t).contiguous(), geometry.scaled(r))

    @torch.no_grad()
    def panorama(self, height=256, width=1024, stride=None, circular=False, eta=0.0, num_inference_steps=50, batch_size=1,
                 generator=None, latents=None, use_graph=True, output_type="pil", return_dict=True):
        """Sample images of height x width PIXELS (multiples of the VAE's scale factor r, as is `stride`; `latents`, if given, is the
        start canvas in latent units): panorama_latents on the canvas of height / r x width / r latents, then decode_panorama.
        output_type as __call__; 'latent' returns the fp32 canvas."""
        self._refuse_dpm("panorama")
        if self.vae is None:
            raise NotImplementedError("this pipeline was built without a VAE: use panorama_latents")
        r = self._vae_ratio()
        for name, v in (("height", height), ("width", width), ("stride", stride)):
            if v is not None and (int(v) % r or int(v) < r):
                raise ValueError(f"panorama: {name} = {v} pixels must be a positive multiple of the VAE's scale factor {r}")
        lstride = None if stride is None else int(stride) // r
        canvas = self.panorama_latents(int(height) // r, int(width) // r, lstride, circular, eta, num_inference_steps, batch_size,
                                       generator, latents, use_graph)
        if output_type == "latent":
            return canvas
        decoded = self.decode_panorama(canvas, self.panorama_geometry(int(height) // r, int(width) // r, lstride, circular))
        return self._images(decoded, output_type, return_dict)

    # ------------------------------------------------------------------------------------------------ outpainting
    @torch.no_grad()
    def outpaint_latents(self, known_canvas, canvas_mask, stride=None, circular=False, num_inference_steps=50, eta=0.0,
                         jump_length=10, jump_n_sample=10, generator=None, latents=None, use_graph=True):
        """RePaint on a MultiDiffusion canvas, in latent space: sample canvases [P, C, Hc, Wc] that agree with `known_canvas` where
        `canvas_mask` [P | 1, 1, Hc, Wc] is 1 and are generated where it is 0 (soft values blend) - a picture around a given crop,
        or a strip of a given panorama repainted.  The canvas is known_canvas's; the windows are panorama_geometry's (`stride`,
        `circular`).  Every evaluation runs the UNet on the windows as one batch, takes RePaint's reverse step per window, fuses
        the steps by the plain mean over the windows that cover an element (panorama_latents), blends in the known content
        noised to the same level and, where the schedule jumps, noises the canvas back up (inpaint_latents).  The schedule is
        DDIMScheduler.outpaint_schedule: every evaluation ends in one afldm_pano_repaint_step, on replayed HIP graphs
        (use_graph), or runs statement by statement in the eager loop below, which makes the same draws from `generator` in the
        same order - the start canvas (unless `latents` [P, C, Hc, Wc] is given), then per evaluation canvas-shaped z_k, z_u, z_b
        where the schedule draws them.  Needs no VAE.  Returns the fp32 canvas; with a hard mask the kept latents are
        `known_canvas` exactly."""
        from .. import ops
        from ..engine import OutpaintEngine
        self._refuse_dpm("outpaint_latents")
        c, s, dev = self.unet.config.in_channels, self.unet.config.sample_size, self.unet.device
        if known_canvas.dim() != 4 or known_canvas.shape[1] != c or known_canvas.shape[2] < s or known_canvas.shape[3] < s:
            raise ValueError(f"outpaint_latents: known_canvas {tuple(known_canvas.shape)}, want [P, {c}, >= {s}, >= {s}]")
        P, _, Hc, Wc = known_canvas.shape
        if canvas_mask.dim() != 4 or tuple(canvas_mask.shape[1:]) != (1, Hc, Wc) or canvas_mask.shape[0] not in (1, P):
            raise ValueError(f"outpaint_latents: canvas_mask {tuple(canvas_mask.shape)}, want [{P} or 1, 1, {Hc}, {Wc}]")
        shape = (P, c, Hc, Wc)
        if latents is not None and tuple(latents.shape) != shape:
            raise ValueError(f"outpaint_latents: latents {tuple(latents.shape)}, want {shape}")
        geom = self.panorama_geometry(Hc, Wc, stride, circular)
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.outpaint_schedule(num_inference_steps, eta, jump_length, jump_n_sample)
        known = known_canvas.to(device=dev, dtype=torch.float32).contiguous()
        mask = canvas_mask.to(device=dev, dtype=torch.float32).contiguous()
        ones = torch.ones(s, s, dtype=torch.float32, device=dev)

        def eager(x, t, row, zs):
            p, q, lo, hi, a, b, cz, k0, k1, u0, u1, _ = row
            zk, zu, zb = zs
            win = ops.window_crop(x, geom)                                    # [P * nwin, C, S, S]
            eps = self.unet(win.to(self.unet.dtype), t).sample.float()
            x0 = torch.clamp(p * win + q * eps, lo, hi)
            unknown = a * ops.window_fuse(x0.contiguous(), ones, geom) + b * ops.window_fuse(eps.contiguous(), ones, geom)
            if zu is not None:
                unknown = unknown + cz * zu
            knownp = k0 * known if zk is None else k0 * known + k1 * zk
            y = mask * knownp + (1 - mask) * unknown
            x = u0 * y if zb is None else u0 * y + u1 * zb
            return x.contiguous()
        return self._sample(sched, shape, generator, latents, use_graph, "_outpaint_engines", eager, OutpaintEngine, P * geom.nwin,
                            known=(known, mask), geometry=geom)

    @torch.no_grad()
    def outpaint(self, image, height, width, top=None, left=None, keep_margin=0, stride=None, circular=False,
                 num_inference_steps=50, eta=0.0, jump_length=10, jump_n_sample=10, generator=None, latents=None, use_graph=True,
                 composite=True, output_type="pil", return_dict=True):
        """Paint the height x width picture around `image` [B, 3, r S, r S] in [-1, 1] (the model's native size, as inpaint takes
        it).  height, width, top, left and stride are PIXELS, multiples of the VAE's scale factor r; (top, left) is the image's
        corner on the canvas, None centres it, and with `circular` the x axis wraps and so does the paste.  The image is encoded
        with the posterior mode times scaling_factor and pasted into a zero canvas of height / r x width / r latents; the canvas
        mask is 1 on that rectangle shrunk by `keep_margin` latents on each side (panorama.place) - the AF-VAE's filters are
        global per plane, so the outermost latents of an encode see the image's opposite edge, and the margin hands them to the
        sampler.  Sampling is outpaint_latents, decoding decode_panorama.  composite: the pixels under the mask are the input's
        exactly, in fp32.  output_type as __call__; 'latent' returns the fp32 canvas."""
        from ..panorama import place
        self._refuse_dpm("outpaint")
        if self.vae is None:
            raise NotImplementedError("this pipeline was built without a VAE: use outpaint_latents")
        r, s, dev = self._vae_ratio(), self.unet.config.sample_size, self.unet.device
        if image.dim() != 4 or tuple(image.shape[1:]) != (3, s * r, s * r):
            raise ValueError(f"outpaint: image {tuple(image.shape)}, want [B, 3, {s * r}, {s * r}]")
        for name, v in (("height", height), ("width", width), ("stride", stride), ("top", top), ("left", left)):
            if v is not None and (int(v) != v or int(v) % r or int(v) < (r if name in ("height", "width", "stride") else 0)):
                raise ValueError(f"outpaint: {name} = {v} pixels must be a {'positive ' if name not in ('top', 'left') else ''}"
                                 f"multiple of the VAE's scale factor {r}")
        Hc, Wc = int(height) // r, int(width) // r
        lstride = None if stride is None else int(stride) // r
        at = place(Hc, Wc, s, None if top is None else int(top) // r, None if left is None else int(left) // r, keep_margin,
                   bool(circular))
        image = image.to(device=dev, dtype=torch.float32)
        z = self._encode_mode(image).float()
        B = image.shape[0]
        rows, cols = torch.tensor(at.rows, device=dev), torch.tensor(at.cols, device=dev)
        known = torch.zeros(B, z.shape[1], Hc, Wc, dtype=torch.float32, device=dev)
        known[:, :, rows[:, None], cols[None, :]] = z
        mask = torch.tensor(at.mask(Hc, Wc), dtype=torch.float32, device=dev)[None, None]
        canvas = self.outpaint_latents(known, mask, lstride, circular, num_inference_steps, eta, jump_length, jump_n_sample,
                                       generator, latents, use_graph)
        if output_type == "latent":
            return canvas
        decoded = self.decode_panorama(canvas, self.panorama_geometry(Hc, Wc, lstride, circular))
        if composite:
            up = torch.arange(r, device=dev)
            prow, pcol = (rows[:, None] * r + up).reshape(-1), (cols[:, None] * r + up).reshape(-1)      # the image's pixels
            pasted = torch.zeros_like(decoded)
            pasted[:, :, prow[:, None], pcol[None, :]] = image
            pmask = mask.repeat_interleave(r, 2).repeat_interleave(r, 3)
            decoded = torch.where(pmask == 1, pasted, decoded)
        return self._images(decoded, output_type, return_dict)

    # ------------------------------------------------------------------------------------------------ high-resolution sampling
    HIRES_MAX_CANVAS = 64           # afldm_hires_step holds a canvas plane in one workgroup's LDS

    @torch.no_grad()
    def hires_latents(self, base_latents, scale=2, stride=None, eta=0.0, num_inference_steps=50, cosine_scale_1=3.0,
                      cosine_scale_2=1.0, cosine_scale_3=1.0, generator=None, use_graph=True):
        """The same kind of image at `scale` times the resolution, in latent space (after DemoFusion, Du et al., CVPR 2024; one
        phase, S -> scale S): `base_latents` [P, C, S, S] are clean latents sampled at the model's own size.  They are upsampled
        (ref = U z0 U^T, the interpolating ideal upsampler afldm_filter_matrix(0, S, scale)), noised with ONE canvas-shaped tensor
        eps_ref to the first level, and the canvas [P, C, scale S, scale S] is denoised through MultiDiffusion windows (the local
        windows of panorama_geometry with `stride`, default S // 2) plus the two things that tie its far ends together: a skip
        residual towards the reference noised with the same eps_ref (weight kappa^cosine_scale_1), and dilated sampling -
        scale^2 more windows per canvas that take every scale-th latent of the whole canvas, whose prediction is mixed with the
        local mean (weight kappa^cosine_scale_2) and whose input is the canvas behind the ideal low-pass of cut-off 1 / scale
        (ilvr_filter; blended in by kappa^cosine_scale_3), under which the scale^2 views are sub-pixel shifts of one image.  A
        cosine scale of None switches its term off; all three None is MultiDiffusion from the noised reference.  The schedule is
        DDIMScheduler.hires_schedule: every evaluation runs the UNet on P (nwin + scale^2) windows and ends in one
        afldm_hires_step, on replayed HIP graphs (use_graph), or runs statement by statement in the eager loop below, which makes
        the same draws from `generator` in the same order - eps_ref in the model's dtype, then one canvas-shaped tensor per
        evaluation whose sigma is not 0.  Needs no VAE.  Returns the fp32 canvas."""
        from .. import ops
        from ..af_libs.ideal_lpf import ilvr_filter
        from ..engine import HiresEngine
        self._refuse_dpm("hires_latents")
        c, s, dev = self.unet.config.in_channels, self.unet.config.sample_size, self.unet.device
        if int(scale) != scale or int(scale) < 2:
            raise ValueError(f"hires_latents: scale = {scale} must be an integer >= 2")
        scale = int(scale)
        Hc = scale * s
        if Hc > self.HIRES_MAX_CANVAS:
            raise ValueError(f"hires_latents: scale {scale} of sample_size {s} is a canvas of {Hc} latents; the limit is "
                             f"{self.HIRES_MAX_CANVAS} (one workgroup holds a canvas plane in LDS)")
        if base_latents.dim() != 4 or tuple(base_latents.shape[1:]) != (c, s, s):
            raise ValueError(f"hires_latents: base_latents {tuple(base_latents.shape)}, want [P, {c}, {s}, {s}]")
        P = base_latents.shape[0]
        shape = (P, c, Hc, Hc)
        geom = self.panorama_geometry(Hc, Hc, s // 2 if stride is None else stride)
        nwin, NW = geom.nwin, geom.nwin + scale * scale
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        sched = self.scheduler.hires_schedule(num_inference_steps, eta, cosine_scale_1, cosine_scale_2, cosine_scale_3)
        k0, k1, f0 = self.scheduler.hires_start(num_inference_steps, cosine_scale_3)
        z0 = ops.to_nhwc(base_latents.to(device=dev, dtype=torch.float32).contiguous())
        ref = ops.to_nchw(ops.af_resample(z0, ops.up_matrix(s, scale, dev)))
        eps_ref = sched.drawer(generator, shape, dev, self.unet.dtype)().to(device=dev, dtype=torch.float32).contiguous()
        start = k0 * ref + k1 * eps_ref
        L = ilvr_filter(Hc, scale).to(device=dev, dtype=torch.float32).contiguous()
        ones = torch.ones(s, s, dtype=torch.float32, device=dev)
        f_in = [f0]                                                           # the low-pass weight of the NEXT evaluation's input

        def eager(x, t, row, zs):
            p, q, lo, hi, a, b, cz, r0, r1, r, g, f = row
            win = ops.hires_windows(x, L, L, f_in[0], geom, scale)            # [P * NW, C, S, S]: local crops, then dilated views
            eps = self.unet(win.to(self.unet.dtype), t).sample.float().reshape(P, NW, c, s, s)
            loc = eps[:, :nwin].reshape(P * nwin, c, s, s).contiguous()
            x0 = torch.clamp(p * win.reshape(P, NW, c, s, s)[:, :nwin].reshape(P * nwin, c, s, s) + q * loc, lo, hi)
            x0m, em = ops.window_fuse(x0.contiguous(), ones, geom), ops.window_fuse(loc, ones, geom)
            if g != 0.0:
                eg = torch.empty_like(x)
                for i in range(scale):
                    for j in range(scale):
                        eg[:, :, i::scale, j::scale] = eps[:, nwin + i * scale + j]
                x0m = (1 - g) * x0m + g * torch.clamp(p * x + q * eg, lo, hi)
                em = (1 - g) * em + g * eg
            x = a * x0m + b * em
            if zs[0] is not None:
                x = x + cz * zs[0]
            if r != 0.0:
                x = r * (r0 * ref + r1 * eps_ref) + (1 - r) * x
            f_in[0] = f
            return x.contiguous()
        return self._sample(sched, shape, generator, start, use_graph, "_hires_engines", eager, HiresEngine, P * NW,
                            known=(ref, eps_ref), geometry=geom, scale=scale)

    @torch.no_grad()
    def hires(self, batch_size=1, scale=2, base_latents=None, stride=None, eta=0.0, num_inference_steps=50, cosine_scale_1=3.0,
              cosine_scale_2=1.0, cosine_scale_3=1.0, generator=None, use_graph=True, output_type="pil", return_dict=True):
        """Sample images at `scale` times the model's resolution: a base sample at the model's own size (this pipeline's
        __call__ with the same eta, step count and generator, unless `base_latents` [P, C, S, S] is given), hires_latents on the
        canvas of scale x sample_size latents, then decode_panorama over the local windows.  `stride` is in PIXELS, a multiple of
        the VAE's scale factor.  output_type as __call__; 'latent' returns the fp32 canvas."""
        self._refuse_dpm("hires")
        if self.vae is None:
            raise NotImplementedError("this pipeline was built without a VAE: use hires_latents")
        r = self._vae_ratio()
        if stride is not None and (int(stride) != stride or int(stride) % r or int(stride) < r):
            raise ValueError(f"hires: stride = {stride} pixels must be a positive multiple of the VAE's scale factor {r}")
        lstride = None if stride is None else int(stride) // r
        if base_latents is None:
            base_latents = self(batch_size=batch_size, generator=generator, eta=eta, num_inference_steps=num_inference_steps,
                                output_type="latent", use_graph=use_graph)
        canvas = self.hires_latents(base_latents, scale, lstride, eta, num_inference_steps, cosine_scale_1, cosine_scale_2,
                                    cosine_scale_3, generator, use_graph)
        if output_type == "latent":
            return canvas
        s = self.unet.config.sample_size
        Hc = int(scale) * s
        decoded = self.decode_panorama(canvas, self.panorama_geometry(Hc, Hc, s // 2 if lstride is None else lstride))
        return self._images(decoded, output_type, return_dict)
