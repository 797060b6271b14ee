"""SamplingServer — continuous batching over SlotEngine (afldm_amd/engine.py): requests of different step counts share the
batch-`slots` graphs, and a slot that finishes is harvested and refilled from the queue while its neighbours go on.

    server = SamplingServer(pipe, slots=64)
    tickets = [server.submit(n, generator=torch.Generator().manual_seed(i)) for i, n in enumerate((20, 50, 35))]
    server.run()
    latents = [t.result() for t in tickets]          # fp32 [1, C, H, W] each, in request order

The host keeps an exact mirror of every slot - whose request it holds and how many evaluations it still needs - so it never
reads the device to schedule.  One turn of an engine is a boundary and a replay group:

    harvest   every slot whose mirror says it is finished, into a free entry of the output ring
    refill    the free slots from the queue, in arrival order, lowest slot first
    group     k = min(steps_per_graph, m) evaluations, m = the SMALLEST remaining count among the occupied slots while requests
              wait (no slot then sits finished while a request could have it), the LARGEST once the queue is empty (frozen slots
              cost nothing more, and no boundary is needed before the last request ends)

The kernels freeze a finished slot, so every grouping gives the same latents; the policy only decides utilisation.  The host
runs ahead of the GPU: a turn only queues work.  Results leave the ring by non-blocking device-to-host copies with one event per
ticket; a ring entry is free again once its ticket has been collected, and a turn that finds the ring full waits for the oldest.

A pipeline whose scheduler is a DPMSolverMultistepScheduler gets engines built with kinds=("ddim", "dpm"): its requests are
DPM-Solver++ ones by default, submit(..., solver="ddim" | "dpm") chooses per request, and both kinds share the batch - every
slot carries its own solver history, and a 20-step DPM request next to 50-step DDIM ones leaves its slot after 20 evaluations.

A server built with kinds that hold "seeded" - kinds=("ddim", "seeded"), or ("ddim", "dpm", "seeded") - builds SeededSlotEngines and
also takes stochastic DDIM requests: submit(n, eta=0.7, seed=s).  Such a request's noise is a function of its seed, the step and
the element (include/afldm_hip_noise.h), so its result is the same in any slot, next to any neighbours, under any grouping.

A server built with kinds that hold "seeded_sdedit" or "seeded_repaint" builds EditSlotEngines and also takes image-conditioned
requests: submit_img2img_latents / submit_img2img (SDEdit with a change map) and submit_inpaint_latents / submit_inpaint (RePaint),
each with a seed.  The request's original or known latents and its map or mask travel with the refill into the slot's own planes,
and every noise it uses - img2img's one fixed noise and RePaint's three per evaluation included - is the counter stream of its seed
(include/afldm_hip_edit.h).  A strength-0.3 edit of 15 evaluations and a RePaint request of 100 share the batch like any others.

engines=2 builds two engines of `slots` slots each on two streams and deals the requests out alternately: two jobs in flight on
one GPU, each filling the other's launch ramps and tails."""
import collections
import contextlib
import inspect

import torch

from .utils import randn_tensor


EDIT_KINDS = ("seeded_sdedit", "seeded_repaint")          # the image-conditioned kinds (EditSlotEngine)


class Ticket:
    """One submitted sample.  done(): its latents have arrived on the host; result(): the fp32 latents [1, C, H, W] (waits for the
    copy if the sample has been harvested, raises if it has not: drive the server with run() or poll())."""

    def __init__(self, server, index, engine, steps, span, latents, seed=0):
        self.server, self.index, self.engine, self.steps, self.seed = server, index, engine, steps, seed
        self._span, self._start, self._ring, self._event, self._latents = span, latents, None, None, None
        self._planes = (None, None)        # an image-conditioned request: (cond, cmask), what its slot's planes are filled with
        self._composite = None             # a request made from an image: (pipeline's composite, image, map or mask) for decode

    def done(self):
        return self._latents is not None or (self._event is not None and self._event.query())

    def result(self):
        if self._latents is None:
            if self._event is None:
                raise RuntimeError(f"Ticket {self.index}: not sampled yet - call SamplingServer.run() or poll()")
            self.server._collect(self)
        self.server._verify(self.engine)
        return self._latents


class SamplingServer:
    def __init__(self, pipe, slots=64, steps_per_graph=5, engines=1, use_graph=True, engine_factory=None, kinds=None,
                 **capacities):
        """pipe: a MyLDMPipeline (its UNet and scheduler config); slots: per engine; kinds: the schedule kinds the engines take
        (SlotEngine's `kinds`; None: ("ddim", "dpm") when pipe.scheduler is a DPMSolverMultistepScheduler, else ("ddim",); kinds
        that hold "seeded" build SeededSlotEngines, which take stochastic requests: submit(n, eta=..., seed=...); kinds that hold
        "seeded_sdedit" or "seeded_repaint" build EditSlotEngines, which also take submit_img2img* and submit_inpaint* requests);
        capacities: SlotEngine's row_capacity, temb_capacity, out_capacity.  engine_factory(i): builds engine i instead (the host
        tests pass a counting fake)."""
        if slots < 1 or engines < 1 or steps_per_graph < 1:
            raise ValueError("SamplingServer: slots, engines and steps_per_graph must be at least 1")
        self.pipe, self.slots, self.steps_per_graph = pipe, int(slots), int(steps_per_graph)
        self.kinds = self.default_kinds(pipe) if kinds is None else tuple(kinds)
        self._edit = any(k in self.kinds for k in EDIT_KINDS)          # refills then carry the request's seed and its planes
        self._seeded = "seeded" in self.kinds or self._edit            # refills then carry the request's seed
        self._streams, self.engines = [], []
        for i in range(engines):
            # one stream per engine when there are several; a single engine works on the caller's current stream
            self._streams.append(torch.cuda.Stream() if engines > 1 and engine_factory is None else None)
            with self._on(i):
                if engine_factory is not None:
                    self.engines.append(engine_factory(i))
                else:
                    from .engine import EditSlotEngine, SeededSlotEngine, SlotEngine
                    cls = EditSlotEngine if self._edit else SeededSlotEngine if self._seeded else SlotEngine
                    self.engines.append(cls(pipe.unet, self.slots, use_graph, self.steps_per_graph, kinds=self.kinds, **capacities))
        if any(s is not None for s in self._streams):
            torch.cuda.synchronize()
        self._queue = [collections.deque() for _ in self.engines]
        self._slot = [[None] * self.slots for _ in self.engines]       # the mirror: None or [ticket, evaluations still to run]
        self._free = [list(range(e.out_capacity)) for e in self.engines]
        self._pending = [collections.deque() for _ in self.engines]    # harvested tickets that still hold a ring entry, oldest first
        self._unchecked = [False] * engines
        self._count = 0
        self.replays = self.evaluations = self.useful = 0              # graph replays, slot evaluations, those of occupied slots

    def _on(self, e):
        s = self._streams[e]
        return contextlib.nullcontext() if s is None else torch.cuda.stream(s)

    # ------------------------------------------------------------------------------------------------ requests
    @staticmethod
    def default_kinds(pipe):
        """What a server built for this pipeline takes: "dpm" schedules too when its scheduler is a DPM-Solver one."""
        from .schedulers.dpmsolver import DPMSolverMultistepScheduler
        return ("ddim", "dpm") if isinstance(pipe.scheduler, DPMSolverMultistepScheduler) else ("ddim",)

    def _ddim(self):
        """A FRESH DDIMScheduler of the pipeline scheduler's config."""
        from .schedulers.ddim import DDIMScheduler
        from .schedulers.dpmsolver import DPMSolverMultistepScheduler
        sched = self.pipe.scheduler
        config = dict(sched.config)
        if isinstance(sched, DPMSolverMultistepScheduler):
            # a DPM config carries the noise schedule, the prediction type and the timestep spacing; what only DDIM has
            # (set_alpha_to_one, ...) is DDIMScheduler's default, and the solver's own settings are not DDIM's to keep
            named = inspect.signature(DDIMScheduler.__init__).parameters
            config = {k: v for k, v in config.items() if k in named}
        return DDIMScheduler.from_config(config)

    def _schedule(self, num_inference_steps, solver=None, eta=0.0):
        """The request's Schedule from a FRESH scheduler of the pipeline scheduler's config: solver None = the pipeline
        scheduler's own class, "ddim" = DDIM (eta = 0), "dpm" = DPM-Solver(++) multistep; eta != 0: DDIM's "seeded" schedule."""
        from .schedulers.dpmsolver import DPMSolverMultistepScheduler
        sched = self.pipe.scheduler
        if solver is None:
            solver = "dpm" if isinstance(sched, DPMSolverMultistepScheduler) and eta == 0.0 else "ddim"
        if solver not in ("ddim", "dpm"):
            raise ValueError(f"SamplingServer: solver {solver!r}: 'ddim', 'dpm' or None (the pipeline scheduler's own)")
        if solver == "dpm":
            return DPMSolverMultistepScheduler.from_config(sched.config).schedule(int(num_inference_steps))
        ddim = self._ddim()
        if eta != 0.0:
            return ddim.seeded_schedule(int(num_inference_steps), eta)
        return ddim.schedule(int(num_inference_steps))

    def submit(self, num_inference_steps=50, generator=None, latents=None, schedule=None, solver=None, eta=0.0, seed=None):
        """Queue ONE sample of `num_inference_steps` steps of `solver` ("ddim": DDIM with eta = 0, "dpm": DPM-Solver(++) multistep,
        None: the pipeline scheduler's own class), or of any Schedule of a kind the engines take given as `schedule`; a kind they
        do not take raises the engine's NotImplementedError.  The start latents are drawn as pipe(batch_size=1, generator=...)
        draws them - randn_tensor([1, C, S, S]) with the caller's generator - unless `latents` [1, C, S, S] is given, and scaled
        by the schedule's init_noise_sigma.
        eta != 0 queues a stochastic DDIM sample (a "seeded" schedule): it needs `seed`, an integer in [0, 2^63) that fixes the
        noise of every step, and a server whose kinds hold "seeded" (otherwise the engine's NotImplementedError); solver must be
        None or "ddim".  With a seed and neither `latents` nor `generator`, the start latents are
        randn_tensor(shape, generator=torch.Generator().manual_seed(seed)).  A "seeded" Schedule given as `schedule` needs a seed too."""
        eta = float(eta)
        if seed is not None and not (isinstance(seed, int) and not isinstance(seed, bool) and 0 <= seed < 2 ** 63):
            raise ValueError(f"SamplingServer.submit: seed {seed!r}, want an integer in [0, 2^63)")
        if eta != 0.0 and solver not in (None, "ddim"):
            raise ValueError(f"SamplingServer.submit: eta = {eta} goes with DDIM, not with solver {solver!r}")
        sched = schedule if schedule is not None else self._schedule(num_inference_steps, solver, eta)
        if sched.kind == "seeded" and seed is None:
            raise ValueError("SamplingServer.submit: a stochastic request (eta != 0) needs seed=: its noise is a function of the seed")
        if sched.kind in EDIT_KINDS:
            raise ValueError(f"SamplingServer.submit: a {sched.kind!r} schedule comes with an image: use submit_img2img_latents or "
                             "submit_inpaint_latents")
        return self._enqueue(sched, generator, latents, seed)

    def _enqueue(self, sched, generator, latents, seed, planes=(None, None)):
        """The ticket of one request on `sched` (its engine takes the schedule first, and may refuse it): start latents as `submit`
        states, `planes` the (cond, cmask) of an image-conditioned request."""
        e = self._count % len(self.engines)
        with self._on(e):
            span = self.engines[e].add_schedule(sched)
        cfg = self.pipe.unet.config
        shape = (1, cfg.in_channels, cfg.sample_size, cfg.sample_size)
        if latents is None:
            if generator is None and seed is not None:
                generator = torch.Generator().manual_seed(seed)
            latents = randn_tensor(shape, generator=generator)
        elif tuple(latents.shape) != shape:
            raise ValueError(f"SamplingServer.submit: latents {tuple(latents.shape)}, want {shape}")
        start = latents.to(torch.float32) * sched.init_noise_sigma
        ticket = Ticket(self, self._count, e, span[1] - span[0], span, start, 0 if seed is None else seed)
        ticket._planes = planes
        if self._streams[e] is not None and any(t is not None and t.is_cuda for t in (start, *planes)):
            # (device tensors made on the caller's stream are read on the engine's at the refill)
            self._streams[e].wait_stream(torch.cuda.current_stream())
        self._count += 1
        if ticket.steps == 0:
            ticket._latents, ticket._start = start.cpu(), None
        else:
            self._queue[e].append(ticket)
        return ticket

    # ------------------------------------------------------------------------------------------------ image-conditioned requests
    @staticmethod
    def _edit_seed(who, seed):
        if not (isinstance(seed, int) and not isinstance(seed, bool) and 0 <= seed < 2 ** 63):
            raise ValueError(f"SamplingServer.{who}: seed {seed!r}, want an integer in [0, 2^63): every noise of the request is a "
                             "function of its seed")
        return seed

    def _edit_planes(self, who, cond, cmask, names):
        """(cond [1, C, S, S], cmask [1, 1, S, S]) as contiguous fp32 on the UNet's device; raises for any other shape."""
        cfg = self.pipe.unet.config
        c, s = cfg.in_channels, cfg.sample_size
        if cond.dim() != 4 or tuple(cond.shape) != (1, c, s, s):
            raise ValueError(f"SamplingServer.{who}: {names[0]} {tuple(cond.shape)}, want {(1, c, s, s)} (one request per call)")
        if cmask.dim() != 4 or tuple(cmask.shape) != (1, 1, s, s):
            raise ValueError(f"SamplingServer.{who}: {names[1]} {tuple(cmask.shape)}, want {(1, 1, s, s)}")
        dev = self.pipe.unet.device
        return (cond.to(device=dev, dtype=torch.float32).contiguous(), cmask.to(device=dev, dtype=torch.float32).contiguous())

    @torch.no_grad()
    def submit_img2img_latents(self, orig_latents, strength=0.6, change_map=None, num_inference_steps=50, eta=0.0, seed=None):
        """Queue ONE image-to-image request in latent space: MyLDMPipeline.img2img_latents' sampler (SDEdit with a per-element
        change map) as a "seeded_sdedit" schedule - the last int(num_inference_steps * strength) timesteps, so that many
        evaluations.  orig_latents [1, C, S, S]; change_map [1, 1, S, S] in [0, 1] or None (all ones).  `seed`, an integer in
        [0, 2^63), fixes every noise: the run's one noise z is the counter stream's slot 1 at ordinal 0 (ops.counter_noise), the
        start is k0_start orig + k1_start z by the row img2img_latents starts from, and with eta != 0 every evaluation's z_u is
        slot 0 at its ordinal.  Needs a server whose kinds hold "seeded_sdedit" (otherwise the engine's NotImplementedError); a
        strength that leaves no evaluation raises the schedule's ValueError, as img2img_latents does."""
        from . import ops
        seed = self._edit_seed("submit_img2img_latents", seed)
        cfg = self.pipe.unet.config
        if change_map is None:
            change_map = torch.ones(1, 1, cfg.sample_size, cfg.sample_size)
        orig, cmap = self._edit_planes("submit_img2img_latents", orig_latents, change_map, ("orig_latents", "change_map"))
        ddim = self._ddim()
        sched = ddim.seeded_sdedit_schedule(int(num_inference_steps), strength, float(eta))
        k0s, k1s = ddim.sdedit_start(int(num_inference_steps), strength)
        dev = orig.device
        z = ops.counter_noise(torch.tensor([seed], dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                              tuple(orig.shape), slot=1)
        zero = torch.zeros_like(orig)
        start = ops.sdedit_step_flat(zero, zero, orig, zero, z, None,
                                     (0.0, 0.0, -float("inf"), float("inf"), 0.0, 0.0, 0.0, k0s, k1s, float("inf")))
        return self._enqueue(sched, None, start, seed, (orig, cmap))

    @torch.no_grad()
    def submit_inpaint_latents(self, known_latents, latent_mask, num_inference_steps=50, eta=0.0, jump_length=10, jump_n_sample=10,
                               seed=None):
        """Queue ONE RePaint request in latent space: MyLDMPipeline.inpaint_latents' sampler as a "seeded_repaint" schedule.
        known_latents [1, C, S, S]; latent_mask [1, 1, S, S], 1 = keep (soft values blend).  `seed`, an integer in [0, 2^63),
        fixes the start latents - randn_tensor(shape, generator=torch.Generator().manual_seed(seed)), as submit draws them - and
        every evaluation's z_k, z_u, z_b: the counter stream's slots 0, 1, 2 at the evaluation's ordinal.  Needs a server whose
        kinds hold "seeded_repaint" (otherwise the engine's NotImplementedError)."""
        seed = self._edit_seed("submit_inpaint_latents", seed)
        known, mask = self._edit_planes("submit_inpaint_latents", known_latents, latent_mask, ("known_latents", "latent_mask"))
        sched = self._ddim().seeded_repaint_schedule(int(num_inference_steps), float(eta), jump_length, jump_n_sample)
        return self._enqueue(sched, None, None, seed, (known, mask))

    @torch.no_grad()
    def submit_img2img(self, image, strength=0.6, change_map=None, num_inference_steps=50, eta=0.0, seed=None, composite=True):
        """Queue ONE image-to-image request from `image` [1, 3, H, W] in [-1, 1] and `change_map` [1, 1, H, W] in [0, 1] or None,
        encoded and pooled exactly as MyLDMPipeline.img2img does; composite: `decode` gives the pixels whose change value is
        exactly 0 back as the input's."""
        seed = self._edit_seed("submit_img2img", seed)
        image, change_map, orig, latent_map = self.pipe._img2img_inputs(image, strength, change_map, "submit_img2img")
        ticket = self.submit_img2img_latents(orig, strength, latent_map, num_inference_steps, eta, seed)
        if composite and change_map is not None:
            ticket._composite = (self.pipe._img2img_composite, image, change_map)
        return ticket

    @torch.no_grad()
    def submit_inpaint(self, image, mask, num_inference_steps=50, eta=0.0, jump_length=10, jump_n_sample=10, seed=None,
                       mask_mode="min", composite=True):
        """Queue ONE RePaint request from `image` [1, 3, H, W] in [-1, 1] and `mask` [1, 1, H, W] (1 = keep), encoded and pooled
        exactly as MyLDMPipeline.inpaint does (mask_mode 'min' or 'mean'); composite: `decode` returns m image + (1 - m) decoded."""
        seed = self._edit_seed("submit_inpaint", seed)
        image, mask, known, latent_mask = self.pipe._inpaint_inputs(image, mask, mask_mode, "submit_inpaint")
        ticket = self.submit_inpaint_latents(known, latent_mask, num_inference_steps, eta, jump_length, jump_n_sample, seed)
        if composite:
            ticket._composite = (self.pipe._inpaint_composite, image, mask)
        return ticket

    # ------------------------------------------------------------------------------------------------ the policy
    def group_size(self, remaining, waiting):
        """Evaluations in the next replay group: `remaining` the counts of the occupied slots (all > 0), `waiting` whether the
        queue holds requests.  See the module docstring."""
        return min(self.steps_per_graph, min(remaining) if waiting else max(remaining))

    def _turn(self, e):
        """One boundary and one replay group of engine e; whether there was anything to do."""
        eng, slots, queue = self.engines[e], self._slot[e], self._queue[e]
        if queue and all(s is None for s in slots):
            # between requests only: a dtype or device change re-allocates the engine's buffers, the output ring among them
            while self._pending[e]:
                self._collect(self._pending[e][0])
            with self._on(e):
                eng.refresh_if_stale()
        finished = [b for b, s in enumerate(slots) if s is not None and s[1] == 0]
        self._reap(e, min(len(finished), eng.out_capacity))
        finished = finished[:len(self._free[e])]        # (a ring smaller than the batch: the others wait a turn, frozen)
        harvests, refills, harvested = {}, {}, {}
        for b in finished:
            ticket = harvested[b] = slots[b][0]
            ticket._ring = harvests[b] = self._free[e].pop()
            self._pending[e].append(ticket)
            slots[b] = None
        for b in range(len(slots)):
            if slots[b] is None and queue:
                ticket = queue.popleft()
                refills[b] = ((ticket._start, *ticket._span) + ((ticket.seed,) if self._seeded else ())
                              + (ticket._planes if self._edit else ()))
                slots[b] = [ticket, ticket.steps]
                ticket._start, ticket._planes = None, (None, None)
        with self._on(e):
            events = eng.exchange(harvests, refills)
            if self._streams[e] is not None:
                # the exchange's copies out of a request's device tensors are queued on the engine's stream, and the last references
                # to them are dropped here: tell the allocator, so that their memory is not handed out again on the stream they
                # were made on before those copies have run
                for refill in refills.values():
                    for t in refill:
                        if torch.is_tensor(t) and t.is_cuda:
                            t.record_stream(self._streams[e])
            for b, ticket in harvested.items():
                ticket._event = events[b]
            remaining = [s[1] for s in slots if s is not None and s[1] > 0]
            if not remaining:
                return any(s is not None for s in slots)
            k = self.group_size(remaining, bool(queue))
            eng.step(k)
        self._unchecked[e] = True
        self.replays += k // self.steps_per_graph + k % self.steps_per_graph
        self.evaluations += k * len(slots)
        for s in slots:
            if s is not None:
                self.useful += min(k, s[1])
                s[1] = max(0, s[1] - k)
        return True

    def _reap(self, e, need):
        """Collect every harvested ticket of engine e whose copy has arrived, then - only if fewer than `need` ring entries are
        free - wait for the oldest ones."""
        for ticket in [t for t in self._pending[e] if t._event is not None and t._event.query()]:
            self._collect(ticket)
        while len(self._free[e]) < need:
            if not self._pending[e]:
                raise RuntimeError(f"SamplingServer: an output ring of {self.engines[e].out_capacity} for {need} finished slots")
            self._collect(self._pending[e][0])

    def _collect(self, ticket):
        e = ticket.engine
        ticket._event.synchronize()
        ticket._latents = self.engines[e].take(ticket._ring)
        self._free[e].append(ticket._ring)
        self._pending[e].remove(ticket)
        ticket._ring = None

    def _verify(self, e):
        """The engine's hand-over error words, read once after the replays that could have set them (DenoiseEngine.check_errors)."""
        if self._unchecked[e]:
            self._unchecked[e] = False
            with self._on(e):
                self.engines[e].check_errors()

    # ------------------------------------------------------------------------------------------------ driving
    def poll(self, max_replays=None):
        """Turns of every engine in rotation until nothing is left to do or `max_replays` graph replays have been queued (the
        turn that reaches the bound is completed).  Returns the number of replays queued.  Does not wait for the GPU."""
        before = self.replays
        busy = True
        while busy and (max_replays is None or self.replays - before < max_replays):
            busy = False
            for e in range(len(self.engines)):
                if self._turn(e):
                    busy = True
        return self.replays - before

    def run(self):
        """Until the queue and the slots are empty and every result is on the host."""
        self.poll()
        for e in range(len(self.engines)):
            while self._pending[e]:
                self._collect(self._pending[e][0])
            self._verify(e)

    def decode(self, tickets, output_type="pil", return_dict=True):
        """The tickets' latents, in the order given, through the pipeline's delivery (MyLDMPipeline._deliver).  A ticket of
        submit_img2img / submit_inpaint(composite=True) gets its pixel composite, as MyLDMPipeline.img2img / inpaint apply it - in
        fp32, so 'pt' is fp32 for a batch that holds such a ticket (the other rows are the decoder's values, unchanged)."""
        unet, pipe = self.pipe.unet, self.pipe
        latents = torch.cat([t.result() for t in tickets]).to(device=unet.device, dtype=unet.dtype)
        if output_type == "latent" or all(t._composite is None for t in tickets):
            return pipe._deliver(latents, output_type, return_dict)
        # a composite is made in fp32, as img2img / inpaint return it, so a batch that holds one is fp32; the rows without one keep
        # the decoder's values
        with torch.no_grad():
            decoded = pipe._decode(latents).float()
            for i, t in enumerate(tickets):
                if t._composite is not None:
                    composite, image, m = t._composite
                    decoded[i:i + 1] = composite(decoded[i:i + 1], image, m)
        return pipe._images(decoded, output_type, return_dict)
