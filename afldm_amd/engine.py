"""DenoiseEngine — the 50-step DDIM loop of the reference (afldm/pipelines/ldm_pipeline.py:103-109)
as ONE captured HIP graph replayed per step.

The reference loop costs, per step, ~1100 dependent kernel launches from Python plus a
`t.item()` device sync.  Here everything the step needs lives in device
memory — the timestep table, the DDIM coefficient table and a step counter the update kernel
increments itself — so a replay needs no host value and no synchronisation:

    step++; t <- t_table[step]; temb <- table[step] (afldm_select_step_row, counter starts at -1: the time-embedding
                                                   MLP and the 27 time_emb_proj layers depend on the timestep only and
                                                   are tabulated once per schedule)
    x_nhwc <- NCHW fp32 latents                   (afldm_nchw_to_nhwc)
    eps    <- UNet(x_nhwc, t)                     (~250 HIP kernels at batch 64, all from libafldm_hip.so)
    lat    <- DDIM(lat, eps, coef[step])          (afldm_ddim_step, in place)

The engine replays a Schedule (schedulers/schedule.py): the timesteps, the coefficient rows and the `kind` of update that
reads them.  A scheduler passed instead is asked for its `.schedule(num_inference_steps)`.  Kind "ddim" (DDIM, the unclipped
I2SB ODE, DDIM inversion) is the last line above.  Kind "dpm" (DPMSolverMultistepScheduler) has [steps, 8] rows and the last
line is afldm_dpm_step, which also keeps the solver's two previous converted outputs in an fp32 history buffer.  Kind "sde"
(DDIM with eta != 0, the stochastic / clipped I2SB bridge) has [steps, 8] rows (p, q, lo, hi, a, b, d, c) and the last line
is afldm_sde_step, which also reads that step's row of an fp32 noise buffer [steps, B, C, H, W].  The noise is drawn per run by
the caller's generator - run(latents, draw=...), the same randn calls the eager loop makes, in the same order - never inside a
capture.  Draws on the CPU (a CPU generator) go through pinned staging: the next replay group's noise is drawn while the GPU
runs the current group.  Kind "repaint" (DDIMScheduler.repaint_schedule: RePaint inpainting) has [steps, 12] rows and the last
line is afldm_repaint_step, which reads up to three noise slots per step of a buffer [steps, 3, B, C, H, W], filled the same way,
and two static per-run tensors, the known latents and the latent mask - run(latents, draw=..., known=(z0, mask)).  The captured
graphs hold the buffers' addresses only, so another image or mask replays the same graphs.  Kind "ilvr"
(DDIMScheduler.ilvr_schedule: ILVR reference-guided sampling) has [steps, 12] rows too and the last line is afldm_ilvr_step - the
one update that is not elementwise: it low-passes a whole (b, c) plane in LDS.  It reads up to two noise slots per step of a buffer
[steps, 2, B, C, H, W] and two static per-run tensors, the reference latents and the [S, S] filter matrix -
run(latents, draw=..., known=(ref, L)); another reference or another cut-off replays the same graphs.

SDEditEngine (kind "sdedit", DDIMScheduler.sdedit_schedule: image-to-image sampling, SDEdit with a change map) has [steps, 12]
rows and afldm_sdedit_step as the last line, which selects per element between the reverse step and the original noised to the
next level with the run's one fixed noise - run(x_start, draw=..., known=(orig, cmap, z)); three static per-run tensors and, only
when eta != 0, a noise buffer [steps, B, C, H, W].

ReversibleEngine (kind "rev", DDIMScheduler.reversible_schedule: the bit-reversible sampler, a two-step DDIM on integers) has
[steps, 4] rows (cx, ce, sign, boot) and afldm_rev_step as the last line.  Its state is a pair of int64 tensors on the grid 2^-32,
rotated in place; `lat` is the fp32 view of the newer one and feeds the next evaluation.  run(start) takes latents or a
ReversibleCode and returns a ReversibleCode; inverting and then sampling (or the reverse) returns the integers it started from.

PanoramaEngine (kind "pano", DDIMScheduler.panorama_schedule: MultiDiffusion) samples a canvas [P, C, Hc, Wc] larger than the UNet's
window: `lat` holds the P * nwin windows of a panorama.Geometry, the canvas is a second fp32 buffer, and the last line of a step is
afldm_pano_step, which applies the "sde" row per window, averages over the windows that cover each canvas element and writes both
the canvas and its crops (the next `lat`).  The noise buffer is canvas-shaped, [steps, P, C, Hc, Wc].

OutpaintEngine (kind "outpaint", DDIMScheduler.outpaint_schedule: RePaint on such a canvas) is PanoramaEngine with
afldm_pano_repaint_step as the last line: the "repaint" row per window, the same averages, then the blend with a known canvas under
a canvas mask - run(canvas, draw=..., known=(known_canvas, canvas_mask)) - and RePaint's jump back up.  The noise buffer is
[steps, 3, P, C, Hc, Wc].

HiresEngine (kind "hires", DDIMScheduler.hires_schedule: a canvas of scale x the window that is ONE image, after DemoFusion) is
PanoramaEngine with scale^2 dilated windows behind the local ones in `lat` and afldm_hires_step as the last line: it mixes the
local means with the dilated window's prediction, pulls the canvas towards the noised upsampled base latents and low-passes the
dilated views of the next input - run(canvas, draw=..., known=(ref, eps_ref)).  The noise buffer is [steps, P, C, Hc, Hc].

PAGEngine (kind "pag", DDIMScheduler.pag_schedule: perturbed-attention guidance) samples B latents with a UNet batch of 2 B: both
halves of `x_nhwc` hold the same latents, the attention blocks named by `sites` run PAGAttnProcessor (the plain block on the first
half, the identity-attention block on the second), and the last line of a step is afldm_pag_step, which reads both halves of eps.

SAGEngine (kind "sag", DDIMScheduler.sag_schedule: self-attention guidance) samples B latents with TWO dependent UNet evaluations
of batch B per step: the first with SAGAttnProcessor at one site, which also writes the attention mass of every key into `mass`;
afldm_sag_degrade turns x, e and the mass into the second evaluation's input; both outputs land in `eps2` [2 B] and the step ends
in afldm_pag_step, unchanged.

CFGEngine (kind "cfg", DDIMScheduler.cfg_schedule: classifier-free guidance over class labels) is the one engine that takes a
class-conditional UNet: the class embedding enters before the SiLU of the time embedding, so instead of copying a tabulated row a
step computes afldm_cond_embed and the projection GEMM per batch row inside the graph, from class rows that are per-run data; the
UNet batch is 2 B (conditional rows, then unconditional rows) and the step ends in afldm_pag_step, unchanged.

SlotEngine has no schedule of its own: every batch row ("slot") walks its own stretch of one device row table with a cursor of
its own, so "ddim" requests of different step counts share the graphs and a finished slot is harvested and refilled between replays
(afldm_slot_select in place of afldm_select_step_row, afldm_slot_step in place of afldm_ddim_step, afldm_slot_exchange at the
boundary); afldm_amd/serving.py drives it.  Built with kinds=("ddim", "dpm") it takes "dpm" requests next to "ddim" ones: a
history per slot and afldm_slot_step_kinds as the update, which reads each row's kind.

SeededEngine (kind "seeded", DDIMScheduler.seeded_schedule) is stochastic DDIM without a noise buffer: afldm_seeded_step makes the
noise in registers from a seed per sample, a device tensor the graphs read.  SeededSlotEngine takes such requests in slots, next to
"ddim" and "dpm" ones: a seed per slot, an ordinal per row and afldm_slot_step_seeded as the update.

PicardEngine (parallel-in-time sampling, ParaDiGMS) walks ONE "ddim" schedule, but a window of its rows at a time: every image keeps
window + 1 states, the UNet evaluates the first `window` of them as one batch with a timestep per row, and the step ends in
afldm_picard_sweep (the recurrence along the window, and how far each estimate moved), afldm_picard_stride (how many states to
accept: the image's cursor moves here and nowhere else, and the next evaluation's rows are gathered) and afldm_picard_slide.  The
host replays until every cursor has reached the end of the schedule.

Structure.  __init__ validates and stores its arguments; _allocate makes every device buffer and is what refresh_if_stale calls
again after unet.to(dtype / device).  A kind is one entry of UPDATES - the update op of ops that ends a step, and a function that
allocates what the kind keeps between steps and returns, per branch, the tensors the op takes between eps and the coefficient
table.  Those functions share _noise (the one noise allocator: the slot count comes from schedule.KINDS, and _fill reads the row
shape and slot layout it recorded), _slice (a branch's batch slice) and _static (the second tensor run(known=...) fills, with its
broadcast rule).  A step is _eps (NCHW latents -> the UNet's output) and _apply (the update); a subclass overrides the half that
differs.  cached_engine keeps the engines (and the harness's samplers) a pipeline has built, one resident entry per slot, and
builds the key from the engine class and its own keyword arguments.
"""
import contextlib
import gc
import os

import torch

from . import ops
from .schedulers.schedule import KINDS, Schedule


@contextlib.contextmanager
def capture_guard():
    """Keep Python's cyclic garbage collector out of a stream capture.  A collection inside the capture can free an unreachable
    CUDAGraph (another engine's, dropped inside a reference cycle), and destroying a graph is not permitted while a stream
    captures: the process aborts.  Collect first, then keep the collector off until the capture ends."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def model_state_key(model):
    """Fingerprint of everything a captured step bakes in: module identities (af_api surgery swaps modules), the
    attention processors (set_unet_attn_processor), and every parameter's storage + in-place version counter
    (load_state_dict copies in place -> _version moves; .to() / .half() re-allocate -> data_ptr moves).  ~1 ms for the
    FFHQ UNet; compared once per DenoiseEngine.reset()."""
    def ver(p):
        try:
            return p._version
        except RuntimeError:          # tensors created under torch.inference_mode() have no version counter
            return -1
    mods = tuple((id(m), id(getattr(m, "processor", None))) for m in model.modules())
    params = tuple((p.data_ptr(), ver(p), p.dtype, str(p.device)) for p in model.parameters())
    bufs = tuple((b.data_ptr(), ver(b), b.dtype, str(b.device)) for b in model.buffers())
    return hash((mods, params, bufs))


def cached_engine(owner, slot, schedule, batch, use_graph, unet, cls=None, build=None, extra=(), **kw):
    """The engine `owner` (a pipeline) keeps in its attribute `slot` for this schedule, batch, use_graph, the UNet's dtype and
    device, the engine class `cls` (default DenoiseEngine) and that class's own keyword arguments `kw` (hashable: what else its
    graphs bake in), built on a miss: cls(unet, schedule, batch, steps, use_graph, **kw).  A slot that holds something else (the
    harness's samplers) passes build() and `extra`: what else identifies it.  A slot is a one-entry dict {key: engine}: a miss
    replaces it, and with it the captured graphs and static buffers of the previous one.  Every field a graph bakes in must be
    in the key: a missed one replays a stale graph."""
    assert (not extra) if build is None else (cls is None and not kw), "cached_engine: either cls and its kw, or build= and extra="
    cls = cls or DenoiseEngine
    key = (batch, len(schedule.timesteps), use_graph, unet.dtype, str(unet.device)) + schedule.key
    key += tuple(extra) if build is not None else (cls.__name__,) + tuple(sorted(kw.items()))
    if key not in owner.__dict__.get(slot, ()):
        made = build() if build is not None else cls(unet, schedule, batch, len(schedule.timesteps), use_graph, **kw)
        owner.__dict__[slot] = {key: made}
    return owner.__dict__[slot][key]


def refuse_class_conditional(unet, who):
    """Every engine but CFGEngine hands the UNet a projection of the timestep alone: on a class-conditional UNet that would
    ignore the labels silently, so it is an error."""
    if getattr(unet, "class_embedding", None) is not None:
        raise ValueError(f"{who}: the UNet is class-conditional (class_embedding); only CFGEngine (MyLDMPipeline.cfg_latents) "
                         "carries class labels")


class DenoiseEngine:
    ONE_BRANCH = False          # an update that needs the whole batch in one launch (PanoramaEngine) takes no parallel branches
    CLASS_CONDITIONAL = False   # CFGEngine: the one engine that takes a class-conditional UNet (and only such a UNet)

    def __init__(self, unet, scheduler, batch_size, num_inference_steps=50, use_graph=True, steps_per_graph=5, branches=1):
        if unet.device.type != "cuda":
            raise RuntimeError("DenoiseEngine needs the UNet on an MI355X ('cuda') device; there is no CPU path")
        if not self.CLASS_CONDITIONAL:
            refuse_class_conditional(unet, type(self).__name__)
        self.unet, self.scheduler = unet, scheduler
        self.schedule = scheduler if isinstance(scheduler, Schedule) else scheduler.schedule(num_inference_steps)
        if len(self.schedule.timesteps) != num_inference_steps:
            raise ValueError(f"DenoiseEngine: a schedule of {len(self.schedule.timesteps)} steps for {num_inference_steps}")
        if self.schedule.kind not in self.UPDATES:
            raise NotImplementedError(f"DenoiseEngine: update_kind {self.schedule.kind!r}")
        self.B, self.n = batch_size, num_inference_steps
        self.timesteps = list(self.schedule.timesteps)
        # a replay boundary costs ~9 us of idle GPU (host launch + graph start): besides the one-step graph a
        # `steps_per_graph`-step graph is captured and used for every full group of steps
        self.steps_per_graph = max(1, int(os.environ.get("AFLDM_STEPS_PER_GRAPH", steps_per_graph)))
        self.use_graph = use_graph
        nb = int(os.environ.get("AFLDM_BRANCHES", branches))
        self.branches = nb if nb > 1 and batch_size % nb == 0 and not self.ONE_BRANCH else 1
        if self.branches > 1:
            from . import trunk
            trunk.block("DenoiseEngine with parallel branches")      # (the experimental cooperative trunk needs the GPU to itself)
        self._allocate()

    def _allocate(self):
        """Every device buffer, in the UNet's current dtype and on its device, and the kind's state; drops the graphs."""
        unet, dev = self.unet, self.unet.device
        c, s = unet.config.in_channels, unet.config.sample_size
        self.t_table = torch.tensor(self.timesteps, dtype=torch.float32).to(dev)
        self.coef = self.schedule.table(dev).reshape(-1).contiguous()
        self.step_idx = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.t_cur = torch.zeros(1, dtype=torch.float32, device=dev)
        self.lat = torch.zeros(self.B, c, s, s, dtype=torch.float32, device=dev)
        self.x_nhwc = torch.empty(self._unet_rows(), s, s, c, dtype=unet.dtype, device=dev)
        self.graph = self.graph_multi = None
        self._tabulate()
        self._model_key = model_state_key(unet)
        self._side = [torch.cuda.Stream() for _ in range(self.branches - 1)]
        # counters of in-kernel reductions / cluster hand-overs: private to this engine (one per branch), so that its
        # captured graphs can replay next to another engine's on a different stream
        self._sync = [ops.new_sync_buffer(dev) for _ in range(self.branches)]
        self.hist = self.noise = self.known = self.mask = self.filter = self._static = None
        self._update, state = self.UPDATES[self.schedule.kind]
        self._state = state(self)

    def _unet_rows(self):
        """Rows of the UNet's batch per step: B, unless an engine evaluates several rows per sample (CFGEngine)."""
        return self.B

    def _tabulate(self):
        """Everything of the UNet that depends on the timestep only (time_proj -> time_embedding -> SiLU -> the 27 time_emb_proj
        layers), tabulated once for the schedule: [steps, sum Cout]; a step copies its row."""
        unet = self.unet
        self.temb_table = torch.cat([unet.temb_projection(t) for t in self.timesteps], 0).contiguous()
        self.temb_row = torch.empty_like(self.temb_table[:1])
        self.temb_slices = unet.temb_slices(self.temb_row)

    def _slice(self, b, *tensors, dim=0):
        """Branch b's batch slice (the batch at `dim`) of each of `tensors`; with one branch, the tensors themselves."""
        per = self.B // self.branches
        return tensors if self.branches == 1 else tuple(t.narrow(dim, b * per, per) for t in tensors)

    def _noise(self, row_shape, only_if_drawn=False):
        """The one noise allocator: an fp32 buffer [steps, *row_shape], or [steps, slots, *row_shape] for a kind of several slots
        (KINDS), filled per run by _fill; what is not drawn keeps zeros and is not read (its coefficient is 0, and 0 * NaN of
        stale memory is not 0).  only_if_drawn: no buffer when no step of the schedule draws (the update then gets no noise
        pointer).  Records the row shape and the slot count for _fill and sets up the pinned staging for CPU draws (one buffer
        per replay group in flight).  Returns one entry per branch: its batch slice of the buffer, or None."""
        slots = KINDS[self.schedule.kind][1]
        self._row, self._stage = (tuple(row_shape), slots), []
        if only_if_drawn and not any(self.schedule.draws):
            return [None] * self.branches
        self.noise = torch.zeros((self.n,) + ((slots,) if slots > 1 else ()) + tuple(row_shape), dtype=torch.float32,
                                 device=self.lat.device)
        return [self._slice(b, self.noise, dim=1 + (slots > 1))[0] for b in range(self.branches)]

    def _no_state(self):
        return [()] * self.branches

    def _dpm_state(self):
        """DPM-Solver history (the two previous converted outputs), one contiguous [2, B / branches, C, H, W] per branch."""
        self.hist = torch.zeros((self.branches, 2, self.B // self.branches) + tuple(self.lat.shape[1:]), dtype=torch.float32,
                                device=self.lat.device)
        return [(self.hist[b],) for b in range(self.branches)]

    def _sde_state(self):
        """One noise row per step."""
        return [(z,) for z in self._noise(self.lat.shape)]

    def _repaint_state(self):
        """Three noise slots per step (z_k, z_u, z_b) and the run's known latents and latent mask (a batch-1 mask is broadcast).
        Every branch takes its batch slice of all three."""
        self.known = torch.zeros_like(self.lat)
        self.mask = torch.zeros((self.B, 1) + tuple(self.lat.shape[2:]), dtype=torch.float32, device=self.lat.device)
        self._static = ("mask", self.mask, True)
        return [self._slice(b, self.known, self.mask) + (z,) for b, z in enumerate(self._noise(self.lat.shape))]

    def _ilvr_state(self):
        """Two noise slots per step (z_k, z_u), the run's reference latents and its [S, S] low-pass matrix (used for both axes).
        Every branch takes its batch slice of the reference and the noise; the filter is shared."""
        self.known = torch.zeros_like(self.lat)
        self.filter = torch.zeros(tuple(self.lat.shape[2:]), dtype=torch.float32, device=self.lat.device)
        self._static = ("filter", self.filter, False)
        return [self._slice(b, self.known) + (z, self.filter, self.filter) for b, z in enumerate(self._noise(self.lat.shape))]

    def _guided_state(self):
        """One noise row per step, only when some step draws (eta != 0): "pag" and "sag"."""
        return [(z,) for z in self._noise(self.lat.shape, only_if_drawn=True)]

    # Schedule.kind -> the update of ops that ends a step, and what allocates the buffers it keeps between steps: it returns one
    # argument tuple per branch, passed between eps and the coefficient table, and sets _static where run() takes known=
    UPDATES = {"ddim": (ops.ddim_step, _no_state), "dpm": (ops.dpm_step, _dpm_state), "sde": (ops.sde_step, _sde_state),
               "repaint": (ops.repaint_step, _repaint_state), "ilvr": (ops.ilvr_step, _ilvr_state)}

    # one denoise step, entirely stream-ordered
    def _step(self):
        # the step counter starts at -1 and is advanced by the first kernel of the step
        ops.select_step_row(self.t_table, self.step_idx, self.t_cur, self.temb_table, self.temb_row, pre_advance=True)
        nb = self.branches
        if nb <= 1:
            self._substep(self.lat, self.x_nhwc)
            return
        # The batch as `nb` independent sub-batches on parallel streams (parallel branches of the captured graph):
        # samples are independent, so the kernels of one branch fill the gaps the other leaves - prologues / epilogues
        # of the large convolutions (one tile per CU: nothing inside a launch overlaps them) and the latency-bound
        # launches of the 8x8 .. 2x2 levels.
        main = torch.cuda.current_stream()
        for i, s in enumerate(self._side):
            s.wait_stream(main)
            with torch.cuda.stream(s):
                self._substep(*self._slice(i + 1, self.lat, self.x_nhwc), branch=i + 1)
        self._substep(*self._slice(0, self.lat, self.x_nhwc))
        for s in self._side:
            main.wait_stream(s)

    def _substep(self, lat, x_nhwc, branch=0):
        with ops.sync_scope(self._sync[branch]):
            self._apply(lat, self._eps(lat, x_nhwc), branch)

    def _eps(self, lat, x_nhwc):
        """The first half of a step: the NCHW fp32 latents through `x_nhwc` to the UNet's output (NHWC, the model's dtype)."""
        ops.to_nhwc(lat, self.unet.dtype, out=x_nhwc)
        return self.unet.forward_nhwc(x_nhwc, self.t_cur, temb_slices=self.temb_slices)

    def _apply(self, lat, eps, branch):
        """The second half: the kind's update, in place."""
        self._update(lat, eps, *self._state[branch], self.coef, self.step_idx, advance=False, out=lat)

    def _capture(self, counts, before_step=None):
        """One captured graph per entry of `counts`, each holding that many steps from the start of the schedule, after ONE
        warm-up step on a side stream.  before_step(i): called on the host before step i is launched or recorded (the harness
        tells its attention processors the timestep).  The engine's state is as before on return."""
        carried = self._carried()                     # the warm-up step shifts the history too
        keep = [t.clone() for t in carried]

        def rewind():
            self._rewind()
            for t, k in zip(carried, keep):
                t.copy_(k)

        def steps(k):
            for i in range(k):
                if before_step is not None:
                    before_step(i)
                self._step()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                 # warm-up: packs weights, fills caches, sizes workspaces
            steps(1)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.check_errors()                           # (the warm-up step ran every hand-over once: free to look, we just synchronised)
        graphs = []
        for k in counts:
            rewind()
            g = torch.cuda.CUDAGraph()
            with capture_guard(), torch.cuda.graph(g):
                steps(k)
            graphs.append(g)
        rewind()
        return graphs

    def _carried(self):
        """The buffers a step reads and overwrites: what _capture puts back after its warm-up step and its captures."""
        return [self.lat] + ([] if self.hist is None else [self.hist])

    def _rewind(self):
        """The step counter back to the start of the schedule (_capture, before every capture and on return)."""
        self.step_idx.fill_(-1)

    def _result(self):
        return self.lat.clone()

    def check_errors(self):
        """Read (and clear) the error words of this engine's sync buffers.  The attention block's in-launch hand-over
        (afldm_attn_block_fused_out, csrc/attnf.hip phase C) gives up after a bounded spin instead of hanging the device and
        then finishes on incomplete data: that must never pass silently.  On a hit the fused tail is switched off
        for the process, this engine's graphs are dropped (the next step re-captures on the two-launch path) and a
        RuntimeError says that the latents of this run are invalid.  Synchronises."""
        sk, ho = ops.sync_errors(self._sync)
        if not (sk or ho):
            return
        self.graph = self.graph_multi = None
        if ho:
            ops._FUSED_ATTN_OUT = False
        raise RuntimeError(
            f"afldm_amd: an in-launch hand-over gave up (split-K word {sk}, hand-over word {ho}: 1 = a workgroup waited out its "
            "cluster, 2 = a cluster straddled XCDs): the latents of this run are INVALID.  The fused attention tail is now off "
            "(two launches per block); run again.  Causes: a CU mask / partitioned device, or many concurrent heavy streams.")

    def refresh_if_stale(self):
        """The captured graphs hold the packed-weight pointers and the time-embedding table of the model AS IT WAS at
        capture: after load_state_dict / .to() / af_api surgery / set_unet_attn_processor they would replay the old
        model (or freed packed tensors).  Re-tabulate and drop the graphs when the model's fingerprint moved
        (ADVICE r02)."""
        key = model_state_key(self.unet)
        if key == self._model_key:
            return False
        from .models.blocks import invalidate_stale_packed
        torch.cuda.synchronize()
        if self.unet.dtype != self.x_nhwc.dtype or self.unet.device != self.x_nhwc.device:
            # .to(dtype / device): every dtype-typed static buffer of the engine is stale, not just the table
            invalidate_stale_packed(self.unet)
            self._allocate()
            return True
        self.graph = self.graph_multi = None
        # in-place parameter edits do not pass through the modules' own hooks; another engine of this model may have repacked
        # (and captured on the new copies) already
        invalidate_stale_packed(self.unet)
        self._retabulate()
        self._model_key = key
        return True

    def _retabulate(self):
        """The time-embedding table of the model as it is now, written in place (the graphs hold its address)."""
        self.temb_table.copy_(torch.cat([self.unet.temb_projection(t) for t in self.timesteps], 0))

    def reset(self, latents):
        """latents: [B, C, H, W] (any device / float dtype); scaled by init_noise_sigma like the reference."""
        self.refresh_if_stale()
        self.lat.copy_(latents.to(device=self.lat.device, dtype=torch.float32) * self.schedule.init_noise_sigma)
        self.step_idx.fill_(-1)
        if self.hist is not None:
            self.hist.zero_()        # the first rows weigh it by 0, but stale memory may hold NaN

    def step(self, k=1):
        if self.use_graph and self.graph is None:
            if self.steps_per_graph > 1:
                self.graph, self.graph_multi = self._capture([1, self.steps_per_graph])
            else:
                self.graph, = self._capture([1])
        if not self.use_graph:
            for _ in range(k):
                self._step()
            return
        while self.graph_multi is not None and k >= self.steps_per_graph:
            self.graph_multi.replay()
            k -= self.steps_per_graph
        for _ in range(k):
            self.graph.replay()

    def _fill(self, k0, k1, draw):
        """Noise rows k0 .. k1 - 1: one draw() per slot a step draws ("sde": one per step at the most, "repaint": up to three - z_k,
        z_u, z_b, "ilvr": up to two - z_k, z_u), in step and slot order.  A CPU draw is copied into pinned staging and on to the
        device with non_blocking (stream-ordered before the replays that read it); the staging buffer is reused only after the
        event behind its previous copy has passed.  A device draw is copied on the stream."""
        shape, slots = self._row                               # as _noise allocated ("pano": the canvas's shape, not lat's)
        rows = [self.noise[k, j] if slots > 1 else self.noise[k] for k in range(k0, k1) for j in self.schedule.slots(k)]
        if not rows:
            return
        stage = None
        for i, row in enumerate(rows):
            z = draw()
            if tuple(z.shape) != shape:
                raise ValueError(f"DenoiseEngine: draw() gave {tuple(z.shape)}, want {shape}")
            if z.device.type != "cpu":
                row.copy_(z)
                continue
            if stage is None:
                if len(self._stage) < 2:
                    self._stage.append((torch.empty((self.steps_per_graph * slots,) + shape,
                                                    dtype=torch.float32, pin_memory=True), torch.cuda.Event()))
                    stage = self._stage[-1]
                else:
                    self._stage.append(self._stage.pop(0))          # the older of the two
                    stage = self._stage[-1]
                    stage[1].synchronize()
            stage[0][i].copy_(z)
            row.copy_(stage[0][i], non_blocking=True)
        if stage is not None:
            stage[1].record()

    def _check_known(self, known):
        """run()'s known=, checked against the static buffers of the kind before anything is written: (z0, extra), or (None, None)
        for a kind that takes none."""
        if (self._static is None) != (known is None):
            raise ValueError("DenoiseEngine: known=(z0, mask) goes with a 'repaint' schedule and known=(ref, L) with an 'ilvr' "
                             "one, and only with those")
        if known is None:
            return None, None
        name, second, broadcast = self._static
        fits = [tuple(second.shape)] + ([(1,) + tuple(second.shape[1:])] if broadcast else [])
        z0, extra = known
        if tuple(z0.shape) != tuple(self.lat.shape) or tuple(extra.shape) not in fits:
            raise ValueError(f"DenoiseEngine: known latents {tuple(z0.shape)} / {name} {tuple(extra.shape)}, want "
                             f"{tuple(self.lat.shape)} / {tuple(second.shape)}" + (" (or batch 1)" if broadcast else ""))
        return z0, extra

    def _set_known(self, z0, extra):
        """run()'s known=, as _check_known returned it, into the static buffers the captured graphs read."""
        self.known.copy_(z0)
        self._static[1].copy_(extra)

    @torch.no_grad()
    def run(self, latents, draw=None, known=None):
        """latents -> the sampled latents (fp32).  An "sde", "repaint" or "ilvr" schedule needs `draw`: a callable returning the next
        noise tensor [B, C, H, W] (on the CPU or on the engine's device, any float dtype), called once per draw in step (and
        slot) order - for a seeded run, the scheduler's own randn_tensor call with the caller's generator (Schedule.drawer).
        A "repaint" schedule also needs known = (z0, mask): the latents to keep [B, C, H, W] and the latent mask [B | 1, 1, H, W]
        (1 = keep), an "ilvr" schedule known = (ref, L): the reference latents [B, C, H, W] and the low-pass matrix [H, H].
        Both are written to the engine's static buffers before the first replay.  `draw` is ignored when the engine has no noise
        buffer (a "pano", "pag" or "sag" schedule none of whose steps draws, "ddim", "dpm")."""
        z0, extra = self._check_known(known)
        self.reset(latents)
        if known is not None:          # (after reset: a dtype or device change re-allocates the static buffers)
            self._set_known(z0, extra)
        if self.noise is None:
            self.step(self.n)
        else:
            if draw is None:
                raise ValueError(f"DenoiseEngine: a stochastic ({self.schedule.kind!r}) schedule needs run(latents, draw=...)")
            # group by replay: while the GPU runs one group, the host draws the next one's noise
            g = self.steps_per_graph if self.use_graph else 1
            self._fill(0, min(g, self.n), draw)
            k = 0
            while k < self.n:
                m = min(g, self.n - k)
                self.step(m)
                k += m
                self._fill(k, min(k + g, self.n), draw)
        out = self._result()
        self.check_errors()                           # one 8-byte read per run: a run whose hand-over failed must not return latents
        return out


class SDEditEngine(DenoiseEngine):
    """Image-to-image sampling on the replayed graphs: SDEdit with a per-element change map (Differential Diffusion).  A step is
    the plain sampler's launch list with afldm_sdedit_step as the last line: an element whose change value is <= the row's
    threshold is held on the original's noised trajectory k0 orig + k1 z - z the run's ONE fixed noise - and every other element
    takes the reverse step.  run(x_start, draw=..., known=(orig, cmap, z)): the original latents and the fixed noise [B, C, S, S]
    and the change map [B | 1, 1, S, S] are per-run static buffers, so another image, map or noise replays the same graphs;
    x_start is k0_start orig + k1_start z (DDIMScheduler.sdedit_start); `draw` returns latent-shaped tensors, one per evaluation
    that draws (eta != 0).  The update is elementwise per sample, so parallel branches work as for the repaint kind."""

    def _sdedit_state(self):
        """The run's original latents, fixed noise and change map (a batch-1 map is broadcast) and one noise row per step, only
        when some step draws (eta != 0).  Every branch takes its batch slice of all four."""
        self.known = torch.zeros_like(self.lat)
        self.zfix = torch.zeros_like(self.lat)
        self.cmap = torch.zeros((self.B, 1) + tuple(self.lat.shape[2:]), dtype=torch.float32, device=self.lat.device)
        self._static = ("cmap", self.cmap, True)
        return [self._slice(b, self.known, self.cmap, self.zfix) + (z,)
                for b, z in enumerate(self._noise(self.lat.shape, only_if_drawn=True))]

    UPDATES = {"sdedit": (ops.sdedit_step, _sdedit_state)}

    def _check_known(self, known):
        if known is None or len(known) != 3:
            raise ValueError("SDEditEngine: run(x_start, draw=..., known=(orig, cmap, z)) needs the original latents, the change map "
                             "and the run's fixed noise")
        orig, cmap, z = known
        want = tuple(self.lat.shape)
        if tuple(orig.shape) != want or tuple(z.shape) != want or tuple(cmap.shape) not in [tuple(self.cmap.shape),
                                                                                           (1,) + tuple(self.cmap.shape[1:])]:
            raise ValueError(f"SDEditEngine: orig {tuple(orig.shape)} / z {tuple(z.shape)} / change map {tuple(cmap.shape)}, want "
                             f"{want} / {want} / {tuple(self.cmap.shape)} (or batch 1)")
        return orig, (cmap, z)

    def _set_known(self, orig, extra):
        cmap, z = extra
        self.known.copy_(orig)
        self.cmap.copy_(cmap)
        self.zfix.copy_(z)


class SeededEngine(DenoiseEngine):
    """Stochastic DDIM without a noise buffer: kind "seeded" (DDIMScheduler.seeded_schedule), whose update afldm_seeded_step makes
    every element's noise in registers from (the sample's seed, the step's ordinal, the element) - Philox-4x32-10 and Box-Muller
    (include/afldm_hip_noise.h).  run(latents, known=seeds): one integer seed per sample, 0 <= seed < 2^63, as a sequence or an
    int64 tensor; they live in a device tensor the captured graphs read, so other seeds replay the same graphs.  Nothing is drawn
    on the host and nothing is staged; a sample's result depends on its own seed and start latents only - not on its batch
    position or on how the steps are grouped into replays.  The update is elementwise per sample, so parallel branches work:
    each passes its slice of the seeds."""

    def _seeded_state(self):
        """The run's seeds, int64 [B]; every branch takes its batch slice."""
        self.seeds = torch.zeros(self.B, dtype=torch.int64, device=self.lat.device)
        return [self._slice(b, self.seeds) for b in range(self.branches)]

    UPDATES = {"seeded": (ops.seeded_step, _seeded_state)}

    def _check_known(self, known):
        if known is None:
            raise ValueError("SeededEngine: run(latents, known=seeds) needs one integer seed per sample")
        return check_seeds(known, self.B, "SeededEngine"), None

    def _set_known(self, seeds, extra):
        self.seeds.copy_(seeds)


def check_seeds(seeds, count, who):
    """`seeds` (a sequence of ints or an integer tensor) as a host int64 tensor [count], every seed in [0, 2^63)."""
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype not in (torch.int64, torch.int32) or seeds.numel() != count:
            raise ValueError(f"{who}: seeds {tuple(seeds.shape)} {seeds.dtype}, want {count} integers")
        host = seeds.detach().reshape(-1).to(device="cpu", dtype=torch.int64)
    else:
        seeds = list(seeds)
        if len(seeds) != count or not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v < 2 ** 63 for v in seeds):
            raise ValueError(f"{who}: seeds {seeds!r}, want {count} integers in [0, 2^63)")
        host = torch.tensor(seeds, dtype=torch.int64)
    if host.numel() and int(host.min()) < 0:
        raise ValueError(f"{who}: a seed is negative; want integers in [0, 2^63)")
    return host


class ReversibleEngine(DenoiseEngine):
    """The bit-reversible sampler on the replayed graphs (kind "rev", DDIMScheduler.reversible_schedule): a step is the plain
    sampler's launch list with afldm_rev_step as the last line.  The state is a pair of int64 tensors on the grid 2^-32 - `near`,
    the level the UNet is evaluated at, and `far`, the level before it - which the update rotates in place at fixed addresses:
    far <- near, near <- far + sign q, with `lat` <- the fp32 view of the new near, the next evaluation's input.  Integer adds of
    the same q undo each other, so a run of the "invert" schedule followed by one of the "sample" schedule (or the reverse)
    returns the integers it started from - provided every evaluation reproduces its bits, which holds for one batch size, dtype,
    set of weights and build of the library (ReversibleCode records them).  run(start) takes fp32 latents - encoded to the grid, one
    state, so the schedule must start with its boot row - or a ReversibleCode - two states, a from_code schedule - and returns a
    ReversibleCode.  `bad` [B] collects, per sample, whether an element was non-finite or left the int64 range; check_errors
    reads it once after the run and raises FloatingPointError naming the samples."""
    ONE_BRANCH = True           # one `bad` word per sample of the whole batch, one pair of state buffers

    def _rev_state(self):
        """The int64 pair and the per-sample trouble flags."""
        self.far = torch.zeros(tuple(self.lat.shape), dtype=torch.int64, device=self.lat.device)
        self.near = torch.zeros_like(self.far)
        self.bad = torch.zeros(self.B, dtype=torch.int32, device=self.lat.device)
        self._capturing = False
        return [(self.bad,)]

    UPDATES = {"rev": (ops.rev_step, _rev_state)}

    def _apply(self, lat, eps, branch):
        self._update(self.far, self.near, eps, *self._state[branch], self.coef, self.step_idx, advance=False, out=lat)

    def _carried(self):
        return [self.lat, self.far, self.near, self.bad]

    def _capture(self, counts, before_step=None):
        self._capturing = True          # (the flags of the warm-up step are put back with the state: they are the run's to report)
        try:
            return super()._capture(counts, before_step)
        finally:
            self._capturing = False

    def reset(self, start):
        """start: fp32-able latents [B, C, H, W] for a schedule with a boot row, or a ReversibleCode for a from_code schedule -
        (X_N, X_N-1) to sample from, (X_1, X_0) to invert."""
        from .reversible import ReversibleCode, decode
        cfg = self.schedule.config
        sampling, from_code = cfg["_rev_direction"] == "sample", cfg["_rev_from_code"]
        if isinstance(start, ReversibleCode) != from_code:
            raise ValueError("ReversibleEngine: a from_code schedule starts from a ReversibleCode, and only such a schedule does")
        self.refresh_if_stale()
        self.bad.zero_()
        if from_code:
            levels = len(self.timesteps) + 1
            if tuple(start.hi.shape) != tuple(self.lat.shape) or start.k != (levels if sampling else 1):
                raise ValueError(f"ReversibleEngine: a code of {tuple(start.hi.shape)} at level {start.k}, want {tuple(self.lat.shape)} "
                                 f"at level {levels if sampling else 1}")
            far, near = (start.hi, start.lo) if sampling else (start.lo, start.hi)
            self.far.copy_(far)
            self.near.copy_(near)
        else:
            x = start.to(device=self.lat.device, dtype=torch.float32) * self.schedule.init_noise_sigma
            ops.rev_encode(x.contiguous(), self.bad, out=self.near)
            self.far.copy_(self.near)          # (the boot row does not read it)
        self.lat.copy_(decode(self.near))
        self.step_idx.fill_(-1)

    def _result(self):
        from . import _lib
        from .reversible import ReversibleCode
        cfg = self.schedule.config
        sampling = cfg["_rev_direction"] == "sample"
        levels = len(self.timesteps) + (1 if cfg["_rev_from_code"] else 0)
        hi, lo = (self.far, self.near) if sampling else (self.near, self.far)
        return ReversibleCode(hi.clone(), lo.clone(), 1 if sampling else levels, cfg["_rev_steps"], None, self.B, self.unet.dtype,
                              self._model_key, _lib.library_hash())

    def check_errors(self):
        """The base class's check, then `bad`: one read per run.  A flagged sample had q = 0 at some element, so its states are not
        on the trajectory: FloatingPointError names the samples; the others are valid, and so is the next run."""
        super().check_errors()
        if self._capturing:
            return
        rows = self.bad.nonzero().flatten().tolist()
        if rows:
            raise FloatingPointError(f"ReversibleEngine: non-finite values or int64 overflow in the latents of batch rows {rows} "
                                     "(their update was skipped at those elements): the states of these rows are INVALID")


class PanoramaEngine(DenoiseEngine):
    """MultiDiffusion on the replayed graphs: P canvases [P, C, Hc, Wc], each seen by the UNet through the nwin windows of
    `geometry` (panorama.Geometry) - batch_size = P * nwin window planes in `lat`, window k of canvas P at entry P * nwin + k.
    A step is the plain sampler's launch list with afldm_pano_step in place of afldm_sde_step.  reset(canvas) writes the canvas and
    crops the windows; run(canvas, draw=...) returns the final canvas, and needs `draw` (canvas-shaped) only when a step draws.
    The geometry is baked into the captured graphs."""
    ONE_BRANCH = True           # the update reads all windows of a canvas

    def __init__(self, unet, scheduler, batch_size, num_inference_steps=50, use_graph=True, steps_per_graph=5, branches=1, *,
                 geometry):
        if geometry is None:
            raise ValueError("PanoramaEngine needs a panorama.Geometry")
        s = unet.config.sample_size
        if geometry.S != s or batch_size % geometry.nwin:
            raise ValueError(f"PanoramaEngine: windows of {geometry.S} for a UNet of sample_size {s}, batch {batch_size} for "
                             f"{geometry.nwin} windows per canvas")
        self.geometry, self.P = geometry, batch_size // geometry.nwin
        super().__init__(unet, scheduler, batch_size, num_inference_steps, use_graph, steps_per_graph, 1)

    def _pano_state(self):
        """The fp32 canvas, MultiDiffusion's plain count average as the window weight, and one canvas-shaped noise row per step,
        only when some step draws (eta != 0)."""
        g, dev = self.geometry, self.unet.device
        self.canvas = torch.zeros(self.P, self.lat.shape[1], g.Hc, g.Wc, dtype=torch.float32, device=dev)
        self.wt = torch.ones(g.S, g.S, dtype=torch.float32, device=dev)
        return [(self._noise(self.canvas.shape, only_if_drawn=True)[0], self.wt, g)]

    UPDATES = {"pano": (ops.pano_step, _pano_state)}

    def _apply(self, lat, eps, branch):
        self._update(self.canvas, eps, *self._state[branch], self.coef, self.step_idx, advance=False, out=self.canvas, windows_out=lat)

    def _carried(self):
        return [self.lat, self.canvas]

    def _result(self):
        return self.canvas.clone()

    def reset(self, canvas):
        """canvas: [P, C, Hc, Wc] (any device / float dtype); scaled by init_noise_sigma, written to the canvas buffer and cropped
        into the windows."""
        if tuple(canvas.shape) != tuple(self.canvas.shape):
            raise ValueError(f"PanoramaEngine: canvas {tuple(canvas.shape)}, want {tuple(self.canvas.shape)}")
        self.refresh_if_stale()
        self.canvas.copy_(canvas.to(device=self.canvas.device, dtype=torch.float32) * self.schedule.init_noise_sigma)
        ops.window_crop(self.canvas, self.geometry, out=self.lat)
        self.step_idx.fill_(-1)


class OutpaintEngine(PanoramaEngine):
    """Outpainting on the replayed graphs: RePaint on a MultiDiffusion canvas.  PanoramaEngine with afldm_pano_repaint_step in
    afldm_pano_step's place: the "repaint" row per window, the means over the covering windows, then RePaint's blend with the
    content to keep and its jump back up, all on the canvas.  run(canvas, draw=..., known=(known_canvas, canvas_mask)): the content
    [P, C, Hc, Wc] and the mask [P | 1, 1, Hc, Wc] (1 = keep) are per-run static buffers, so another image or mask replays the
    same graphs; `draw` returns canvas-shaped tensors, up to three per evaluation (z_k, z_u, z_b)."""

    def _outpaint_state(self):
        """The fp32 canvas, the count average as the window weight, the run's known canvas and canvas mask (a batch-1 mask is
        broadcast) and three canvas-shaped noise slots per step."""
        g, dev = self.geometry, self.unet.device
        self.canvas = torch.zeros(self.P, self.lat.shape[1], g.Hc, g.Wc, dtype=torch.float32, device=dev)
        self.wt = torch.ones(g.S, g.S, dtype=torch.float32, device=dev)
        self.known = torch.zeros_like(self.canvas)
        self.mask = torch.zeros(self.P, 1, g.Hc, g.Wc, dtype=torch.float32, device=dev)
        self._static = ("mask", self.mask, True)
        return [(self.known, self.mask, self._noise(self.canvas.shape)[0], self.wt, g)]

    UPDATES = {"outpaint": (ops.pano_repaint_step, _outpaint_state)}

    def _check_known(self, known):
        if known is None:
            raise ValueError("OutpaintEngine: run(canvas, draw=..., known=(known_canvas, canvas_mask)) needs the content to keep")
        z0, mask = known
        want = tuple(self.canvas.shape)
        if tuple(z0.shape) != want or tuple(mask.shape) not in [tuple(self.mask.shape), (1,) + tuple(self.mask.shape[1:])]:
            raise ValueError(f"OutpaintEngine: known canvas {tuple(z0.shape)} / mask {tuple(mask.shape)}, want {want} / "
                             f"{tuple(self.mask.shape)} (or batch 1)")
        return z0, mask


class HiresEngine(PanoramaEngine):
    """High-resolution sampling on the replayed graphs (after DemoFusion): P square canvases of scale x the UNet's window, each
    seen through NW = nwin + scale^2 windows - the nwin local windows of `geometry`, then the scale^2 dilated windows, which take
    every scale-th latent of the whole canvas - batch_size = P * NW planes in `lat`.  A step is PanoramaEngine's with
    afldm_hires_step as the last line: the local means mixed with the dilated prediction, the reverse step, the skip residual
    towards the noised reference, and the next UNet input with its dilated views low-passed.  run(canvas, draw=...,
    known=(ref, eps_ref)): the upsampled base latents and the run's noise tensor, both [P, C, Hc, Hc], are per-run static
    buffers, so another base image replays the same graphs; the low-pass L = ilvr_filter(Hc, scale) and the window weight are
    engine state.  reset(canvas) writes the canvas and makes the first UNet input with the schedule's f_0
    (afldm_hires_windows).  Geometry and scale are baked into the captured graphs."""

    def __init__(self, unet, scheduler, batch_size, num_inference_steps=50, use_graph=True, steps_per_graph=5, branches=1, *,
                 geometry, scale):
        if geometry is None or scale is None:
            raise ValueError("HiresEngine needs a panorama.Geometry and the scale")
        s, scale = unet.config.sample_size, int(scale)
        per = geometry.nwin + scale * scale
        if (geometry.S != s or scale < 1 or geometry.Hc != scale * s or geometry.Wc != scale * s or geometry.wrap_y or geometry.wrap_x
                or batch_size % per):
            raise ValueError(f"HiresEngine: windows of {geometry.S} on a {geometry.Hc} x {geometry.Wc} canvas for a UNet of sample_size "
                             f"{s} at scale {scale} (want a square canvas of scale x sample_size that does not wrap), batch "
                             f"{batch_size} for {geometry.nwin} + {scale * scale} windows per canvas")
        self.geometry, self.scale, self.P = geometry, scale, batch_size // per
        DenoiseEngine.__init__(self, unet, scheduler, batch_size, num_inference_steps, use_graph, steps_per_graph, 1)

    def _hires_state(self):
        """The fp32 canvas, the count average as the window weight, the run's reference and noise canvases, the ideal low-pass of
        cut-off 1 / scale on the canvas's plane, and one canvas-shaped noise row per step, only when some step draws."""
        from .af_libs.ideal_lpf import ilvr_filter
        from .schedulers.ddim import hires_kappa
        g, dev = self.geometry, self.unet.device
        self.canvas = torch.zeros(self.P, self.lat.shape[1], g.Hc, g.Wc, dtype=torch.float32, device=dev)
        self.wt = torch.ones(g.S, g.S, dtype=torch.float32, device=dev)
        self.known = torch.zeros_like(self.canvas)
        self.eps_ref = torch.zeros_like(self.canvas)
        self.filter = ilvr_filter(g.Hc, self.scale).to(device=dev, dtype=torch.float32).contiguous()
        self._static = ("eps_ref", self.eps_ref, False)
        cfg = self.schedule.config          # f_0 of DDIMScheduler.hires_start: how far the FIRST input's dilated views are low-passed
        self.f0 = hires_kappa(self.timesteps[0], cfg["num_train_timesteps"], cfg["_hires_cosine_scale_3"])
        return [(self.known, self.eps_ref, self._noise(self.canvas.shape, only_if_drawn=True)[0], self.wt, self.filter, self.filter,
                 g, self.scale)]

    UPDATES = {"hires": (ops.hires_step, _hires_state)}

    def _check_known(self, known):
        if known is None:
            raise ValueError("HiresEngine: run(canvas, draw=..., known=(ref, eps_ref)) needs the upsampled reference and its noise")
        ref, eps_ref = known
        want = tuple(self.canvas.shape)
        if tuple(ref.shape) != want or tuple(eps_ref.shape) != want:
            raise ValueError(f"HiresEngine: ref {tuple(ref.shape)} / eps_ref {tuple(eps_ref.shape)}, want {want} for both")
        return ref, eps_ref

    def reset(self, canvas):
        """canvas: [P, C, Hc, Hc] (any device / float dtype), the noised upsampled reference; scaled by init_noise_sigma, written
        to the canvas buffer and turned into the first UNet input."""
        if tuple(canvas.shape) != tuple(self.canvas.shape):
            raise ValueError(f"HiresEngine: canvas {tuple(canvas.shape)}, want {tuple(self.canvas.shape)}")
        self.refresh_if_stale()
        self.canvas.copy_(canvas.to(device=self.canvas.device, dtype=torch.float32) * self.schedule.init_noise_sigma)
        ops.hires_windows(self.canvas, self.filter, self.filter, self.f0, self.geometry, self.scale, out=self.lat)
        self.step_idx.fill_(-1)


@contextlib.contextmanager
def pag_processors(unet, sites):
    """PAGAttnProcessor on the attention modules `sites` names (module paths), the processors found there put back on the way
    out, also on an exception."""
    from .models.blocks import PAGAttnProcessor
    mods = dict(unet.named_modules())
    found = [(mods[name], mods[name].processor) for name in sites]
    try:
        for m, _ in found:
            m.processor = PAGAttnProcessor()
        yield
    finally:
        for m, old in found:
            m.processor = old


class PAGEngine(DenoiseEngine):
    """Perturbed-attention guidance on the replayed graphs: `lat` [B] are the latents, `x_nhwc` [2 B] the UNet's input - the same
    latents twice - and ONE forward_nhwc evaluates the UNet (rows 0 .. B-1) and the perturbed UNet (rows B .. 2B-1), whose
    attention blocks at `sites` (names as the keys of get_unet_attn_processors) use the identity attention map.  A step is the
    plain sampler's launch list at batch 2 B with afldm_pag_step in place of afldm_sde_step.  PAGAttnProcessor is installed on
    the sites around every warm-up, capture and eager step and the previous processors are put back afterwards, also on an
    exception: outside a call the UNet is as it was found.  The sites are baked into the captured graphs."""
    ONE_BRANCH = True           # the update reads both halves of eps

    def __init__(self, unet, scheduler, batch_size, num_inference_steps=50, use_graph=True, steps_per_graph=5, branches=1, *, sites):
        if sites is None:
            raise ValueError("PAGEngine needs the attention sites to perturb")
        self.sites = tuple(sites)
        super().__init__(unet, scheduler, batch_size, num_inference_steps, use_graph, steps_per_graph, 1)

    def _allocate(self):
        super()._allocate()
        self.x_nhwc = torch.empty((2 * self.B,) + tuple(self.x_nhwc.shape[1:]), dtype=self.unet.dtype, device=self.unet.device)

    UPDATES = {"pag": (ops.pag_step, DenoiseEngine._guided_state)}

    def perturbed(self):
        return pag_processors(self.unet, self.sites)

    def _eps(self, lat, x_nhwc):
        ops.to_nhwc(lat, self.unet.dtype, out=x_nhwc[:self.B])
        ops.to_nhwc(lat, self.unet.dtype, out=x_nhwc[self.B:])
        return self.unet.forward_nhwc(x_nhwc, self.t_cur, temb_slices=self.temb_slices)

    def _capture(self, counts, before_step=None):
        with self.perturbed():
            return super()._capture(counts, before_step)

    def step(self, k=1):
        if self.use_graph and self.graph is not None:
            return super().step(k)          # replays only: the graphs hold the perturbed launch list
        with self.perturbed():
            super().step(k)


class CFGEngine(DenoiseEngine):
    """Class-conditional sampling with classifier-free guidance on the replayed graphs - the one engine that takes a
    class-conditional UNet.  diffusers adds the class embedding to the time embedding BEFORE the SiLU in front of the time_emb_proj
    layers, so the projection is neither a per-step row nor a sum of a step part and a class part: the engine tabulates
    `emb_table` [n, D], time_embedding's output per step before the SiLU, holds the run's class rows as DATA in `class_rows`
    [R, D], and a step is

        afldm_select_timestep (the one place the counter moves); afldm_cond_embed -> `act` [R, D]; the projection GEMM over all
        time_emb_proj layers -> `temb_rows` [R, sum Cout], read by the resnets with a row stride; to_nhwc; forward_nhwc; the update

    all inside the captured graphs, which hold the class rows' address only: other labels replay the same graphs.
    guided (kind "cfg", DDIMScheduler.cfg_schedule): R = 2 B - rows 0 .. B-1 conditional, rows B .. 2B-1 unconditional, both
    halves of `x_nhwc` the same latents - and the update is afldm_pag_step with s = guidance_scale - 1, so sigma(e) of
    guidance_rescale is the conditional prediction's.  Not guided (a plain "ddim" or "sde" schedule: guidance_scale = 1): R = B
    and the scheduler's own update.  run(latents, draw=..., known=class_rows): the rows [R, D] (any float dtype, as
    UNet2DModel.class_embed returns them, the unconditional half behind the conditional one) are copied in before the first
    replay; known=None reuses the rows of the previous run (set_class_rows)."""
    ONE_BRANCH = True           # the update reads both halves of eps; one projection GEMM for the whole batch
    CLASS_CONDITIONAL = True

    def __init__(self, unet, scheduler, batch_size, num_inference_steps=50, use_graph=True, steps_per_graph=5, branches=1, *, guided):
        if getattr(unet, "class_embedding", None) is None:
            raise ValueError("CFGEngine needs a class-conditional UNet (num_class_embeds, or class_embed_type='identity')")
        kind = (scheduler if isinstance(scheduler, Schedule) else scheduler.schedule(num_inference_steps)).kind
        if guided is None or bool(guided) != (kind == "cfg"):
            raise ValueError(f"CFGEngine: guided = {guided} with a schedule of kind {kind!r}: a 'cfg' schedule is guided (2 B UNet rows), "
                             "a plain one is not")
        self.guided, self.R = bool(guided), (2 if guided else 1) * int(batch_size)
        self._rows_given = None
        super().__init__(unet, scheduler, batch_size, num_inference_steps, use_graph, steps_per_graph, 1)

    UPDATES = {"cfg": (ops.pag_step, DenoiseEngine._guided_state), "ddim": DenoiseEngine.UPDATES["ddim"],
               "sde": DenoiseEngine.UPDATES["sde"]}

    def _tabulate(self):
        """The time embeddings per step BEFORE the SiLU, and the per-row buffers of a step."""
        unet, dev = self.unet, self.unet.device
        self.emb_table = torch.cat([unet.time_embedding_row(t) for t in self.timesteps], 0).contiguous()
        D, width = self.emb_table.shape[1], unet._temb_weights(unet.dtype)[3]
        self.class_rows = torch.zeros(self.R, D, dtype=unet.dtype, device=dev)
        self.act = torch.zeros(self.R, D, dtype=unet.dtype, device=dev)
        self.temb_rows = torch.zeros(self.R, width, dtype=unet.dtype, device=dev)
        self.temb_slices = unet.temb_slices(self.temb_rows, per_sample=True)

    def _retabulate(self):
        self.emb_table.copy_(torch.cat([self.unet.time_embedding_row(t) for t in self.timesteps], 0))

    def _unet_rows(self):
        return self.R

    def _allocate(self):
        super()._allocate()
        self._static = ("class_rows", self.class_rows, False)

    def _step(self):
        ops.select_timestep(self.t_table, self.step_idx, self.t_cur, pre_advance=True)
        ops.cond_embed(self.emb_table, self.step_idx, self.class_rows, out=self.act)
        w, b, _, _ = self.unet._temb_weights(self.unet.dtype)
        with ops.sync_scope(self._sync[0]):
            ops.conv2d(self.act, w, b, out=self.temb_rows)
        self._substep(self.lat, self.x_nhwc)

    def _eps(self, lat, x_nhwc):
        ops.to_nhwc(lat, self.unet.dtype, out=x_nhwc[:self.B])
        if self.guided:
            ops.to_nhwc(lat, self.unet.dtype, out=x_nhwc[self.B:])
        return self.unet.forward_nhwc(x_nhwc, self.t_cur, temb_slices=self.temb_slices)

    def set_class_rows(self, rows):
        """The class rows [R, D] of the next runs: a copy is kept (the caller's tensor may change afterwards) and written into the
        static buffer by run, after its reset."""
        if not torch.is_tensor(rows) or tuple(rows.shape) != tuple(self.class_rows.shape) or not rows.is_floating_point():
            got = f"{rows.dtype} {tuple(rows.shape)}" if torch.is_tensor(rows) else type(rows).__name__
            raise ValueError(f"CFGEngine: class rows {got}, want a float tensor {tuple(self.class_rows.shape)} "
                             + ("(conditional rows, then unconditional rows)" if self.guided else "(one row per sample)"))
        self._rows_given = rows.detach().clone()

    def _check_known(self, known):
        if known is not None:
            self.set_class_rows(known)
        if self._rows_given is None:
            raise ValueError("CFGEngine: run(latents, draw=..., known=class_rows) needs the class rows (UNet2DModel.class_embed)")
        return self._rows_given, None

    def _set_known(self, rows, extra):
        self.class_rows.copy_(rows)

    @torch.no_grad()
    def run(self, latents, draw=None, known=None):
        """As DenoiseEngine.run; known = the class rows [R, D], or None to keep the previous run's."""
        return super().run(latents, draw, known if known is not None else self._rows_given)


@contextlib.contextmanager
def sag_processor(unet, site, mass=None):
    """SAGAttnProcessor on the attention module `site` names (a module path), writing into `mass` (or into a tensor of its own
    per call); yields the processor.  The processor found there is put back on the way out, also on an exception."""
    from .models.blocks import SAGAttnProcessor
    mod = dict(unet.named_modules())[site]
    old = mod.processor
    proc = SAGAttnProcessor(mass)
    try:
        mod.processor = proc
        yield proc
    finally:
        mod.processor = old


class SAGEngine(DenoiseEngine):
    """Self-attention guidance on the replayed graphs.  A step: to_nhwc; forward_nhwc with SAGAttnProcessor at `site` (the
    attention mass per key goes to `mass` [B, T]); afldm_sag_degrade (x, e, mass -> `x_nhwc`, the degraded input, NHWC in the
    model dtype); forward_nhwc with the processors as found; both outputs in `eps2` [2 B, H, W, C]; afldm_pag_step.  The second
    evaluation depends on the first, so the two cannot share a batch (PAGEngine's can).  The processor is installed around every
    warm-up, capture and eager step and the one found is put back afterwards, also on an exception: outside a call the UNet is
    as it was found.  Site, taps and boundary are baked into the captured graphs."""
    ONE_BRANCH = True           # the update reads both halves of eps2

    def __init__(self, unet, scheduler, batch_size, num_inference_steps=50, use_graph=True, steps_per_graph=5, branches=1, *,
                 site, taps, boundary):
        if site is None or taps is None or boundary is None:
            raise ValueError("SAGEngine needs the attention site, the blur taps and the boundary")
        mod = dict(unet.named_modules()).get(site)
        if mod is None or not hasattr(mod, "processor"):
            raise ValueError(f"SAGEngine: {site!r} names no attention module")
        self.site, self.taps, self.boundary = site, tuple(float(t) for t in taps), boundary
        super().__init__(unet, scheduler, batch_size, num_inference_steps, use_graph, steps_per_graph, 1)

    def _allocate(self):
        super()._allocate()
        self.mass = None            # [B, T] fp32, made by the warm-up (or first eager) step, which knows the site's T
        self.eps2 = torch.zeros((2 * self.B,) + tuple(self.x_nhwc.shape[1:]), dtype=self.unet.dtype, device=self.unet.device)

    UPDATES = {"sag": (ops.pag_step, DenoiseEngine._guided_state)}

    def _eps(self, lat, x_nhwc):
        B = self.B
        ops.to_nhwc(lat, self.unet.dtype, out=x_nhwc)
        with sag_processor(self.unet, self.site, self.mass) as proc:
            e = self.unet.forward_nhwc(x_nhwc, self.t_cur, temb_slices=self.temb_slices)
        if proc.mass is None:
            raise RuntimeError(f"SAGEngine: the attention module {self.site!r} was not evaluated")
        self.mass = proc.mass       # (the first step outside a capture makes it; from then on the processor writes into it)
        self.eps2[:B].copy_(e)
        ops.sag_degrade(lat, self.eps2[:B], self.mass, self.taps, self.boundary, self.coef, self.step_idx, out=x_nhwc)
        self.eps2[B:].copy_(self.unet.forward_nhwc(x_nhwc, self.t_cur, temb_slices=self.temb_slices))
        return self.eps2


class SlotTable:
    """The host's record of a SlotEngine's row table: the rows of every schedule added so far, each stored once under
    `schedule.key`, and the distinct timesteps they use in the order of the time-embedding table.  Plain Python - what the
    serving layer's host tests run against; SlotEngine uploads what `add` appends."""

    KIND_CODES = {"ddim": 0, "dpm": 1}                     # what afldm_slot_step_kinds reads in row_kind

    def __init__(self, row_capacity, temb_capacity, kinds=("ddim",)):
        self.R, self.T = int(row_capacity), int(temb_capacity)
        self.kinds = tuple(dict.fromkeys(kinds))
        unknown = [k for k in self.kinds if k not in self.KIND_CODES]
        if unknown or not self.kinds:
            raise ValueError(f"SlotTable: kinds {tuple(kinds)!r}: slots know {tuple(self.KIND_CODES)} and need at least one")
        self.coef, self.t, self.temb = [], [], []          # per row: the schedule's own row tuple, the timestep, its time-embedding row
        self.kind = []                                     # per row: its kind's code
        self.timesteps, self._index = [], {}               # per time-embedding row: its timestep; timestep -> row
        self.spans = {}                                    # schedule.key -> (begin, end)

    def add(self, schedule):
        """(begin, end) of the schedule's rows, appended (with its unseen timesteps) on the first call for this key.  Raises
        NotImplementedError for a kind that is not among the table's `kinds` and RuntimeError when a table is full; a refused
        schedule leaves the tables as they were."""
        if schedule.kind not in self.kinds:
            if self.kinds == ("ddim",):
                raise NotImplementedError(f"SlotEngine: update_kind {schedule.kind!r}: slots take 'ddim' schedules only (the other "
                                          "kinds need a noise feed or a history per slot; kinds=('ddim', 'dpm') adds the history)")
            takes = " and ".join(repr(k) for k in sorted(self.kinds, key=lambda k: k == "ddim"))          # ('ddim' last)
            raise NotImplementedError(f"SlotEngine: update_kind {schedule.kind!r}: slots take {takes} schedules only (the "
                                      "other kinds need a noise feed or a second evaluation per slot)")
        if schedule.key in self.spans:
            return self.spans[schedule.key]
        unseen = [t for t in dict.fromkeys(schedule.timesteps) if t not in self._index]
        begin, n = len(self.t), len(schedule.timesteps)
        if begin + n > self.R:
            raise RuntimeError(f"SlotEngine: the row table is full ({begin} of {self.R} rows used, {n} more asked for): build the "
                               "engine with a larger row_capacity")
        if len(self.timesteps) + len(unseen) > self.T:
            raise RuntimeError(f"SlotEngine: the time-embedding table is full ({len(self.timesteps)} of {self.T} rows used, "
                               f"{len(unseen)} more asked for): build the engine with a larger temb_capacity")
        for t in unseen:
            self._index[t] = len(self.timesteps)
            self.timesteps.append(t)
        for t, row in zip(schedule.timesteps, schedule.rows):
            self.coef.append(tuple(row))
            self.kind.append(self.KIND_CODES[schedule.kind])
            self.t.append(float(t))
            self.temb.append(self._index[t])
        self.spans[schedule.key] = (begin, begin + n)
        return self.spans[schedule.key]


class SlotEngine(DenoiseEngine):
    """Continuous batching on the replayed graphs: every batch row ("slot") has its own cursor (pos, end) into one row table on
    the device, so requests of different schedules share a batch and a slot that finishes is harvested and refilled between
    replays while its neighbours go on.  A step is the plain sampler's launch list with afldm_slot_select in place of
    afldm_select_step_row (it advances the cursors of the active slots and gathers one time-embedding row per slot, which the
    UNet reads with a row stride) and afldm_slot_step in place of afldm_ddim_step (each active slot's own coefficient row; a
    finished or empty slot is frozen: evaluated, but not written).  So any grouping of steps into replays gives the same
    latents; grouping only affects utilisation, and is the serving layer's business (afldm_amd/serving.py).

    add_schedule(schedule) -> (begin, end) stores a schedule's rows once per `schedule.key`; the tables have fixed capacities and
    fixed addresses, and are only appended to.  kinds: the schedule kinds the engine takes - ("ddim",) by default; with
    ("ddim", "dpm") DPM-Solver++ requests share the batch with DDIM ones: the rows are 8 wide with a kind code each, every slot
    has its own two history planes (`hist` [2, B, C, S, S], addressed by the slot like its latents, carried by _capture) and
    the update is afldm_slot_step_kinds, which gives a "ddim" slot afldm_ddim_step's bits and a "dpm" slot afldm_dpm_step's.
    exchange(harvests, refills) is the boundary between replays: one afldm_slot_exchange launch behind non-blocking uploads of the command buffer and the fresh latents from pinned
    staging, then one non-blocking device-to-host copy per harvested slot out of the output ring, each with its event.
    The engine has no schedule of its own: reset / run are the base class's and do not apply."""
    ONE_BRANCH = True           # one cursor table, one select launch: no parallel branches
    TABLE = SlotTable           # the host's record of the row table (SeededSlotEngine: SeededSlotTable)
    ROW_WIDTH = 8               # floats per row once the table holds more than "ddim" rows (EditSlotEngine: 12)

    def __init__(self, unet, batch_size, use_graph=True, steps_per_graph=5, *, row_capacity=1024, temb_capacity=256,
                 out_capacity=None, kinds=("ddim",)):
        if unet.device.type != "cuda":
            raise RuntimeError("SlotEngine needs the UNet on an MI355X ('cuda') device; there is no CPU path")
        refuse_class_conditional(unet, "SlotEngine")
        odd = sorted({type(m.processor).__name__ for m in unet.modules() if hasattr(m, "processor")} - {"AttnProcessor2_0"})
        if odd:
            raise ValueError(f"SlotEngine: the UNet has attention processors {odd}; slots need the plain one")
        self.unet, self.scheduler, self.schedule = unet, None, None
        self.B, self.branches, self.use_graph = int(batch_size), 1, use_graph
        self.steps_per_graph = max(1, int(os.environ.get("AFLDM_STEPS_PER_GRAPH", steps_per_graph)))
        self.table = self.TABLE(row_capacity, temb_capacity, kinds)
        self.out_capacity = 2 * self.B if out_capacity is None else int(out_capacity)
        if self.out_capacity < 1:
            raise ValueError("SlotEngine: out_capacity must be at least 1")
        self._busy = set()
        self._allocate()

    timesteps = property(lambda self: self.table.timesteps)

    def _allocate(self):
        """Every device buffer in the UNet's current dtype and on its device, every slot empty, the tables filled from the
        host's record; drops the graphs."""
        unet, dev, B, tb = self.unet, self.unet.device, self.B, self.table
        c, s = unet.config.in_channels, unet.config.sample_size
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.lat = torch.zeros(B, c, s, s, **f32)
        self.x_nhwc = torch.empty(B, s, s, c, dtype=unet.dtype, device=dev)
        self.graph = self.graph_multi = None
        # per slot: the cursor, one past the last row, this step's activity flag and timestep, and this step's row of projections
        self.pos, self.end, self.active = torch.full((B,), -1, **i32), torch.zeros(B, **i32), torch.zeros(B, **i32)
        self.t_cur = torch.zeros(B, **f32)
        width = unet._temb_weights(unet.dtype)[3]               # sum Cout of the time_emb_proj layers
        self.temb_table = torch.zeros(tb.T, width, dtype=unet.dtype, device=dev)
        self.temb_rows = torch.zeros(B, width, dtype=unet.dtype, device=dev)       # (zeros: a never-filled slot evaluates finite)
        self.temb_slices = unet.temb_slices(self.temb_rows, per_sample=True)
        # one update per engine: a table of "ddim" rows alone keeps the 4-wide rows of afldm_slot_step; any other set of kinds takes
        # 8-wide rows ("ddim" rows padded with zeros), a kind code per row and a history per slot (afldm_slot_step_kinds)
        self._by_kind = tb.kinds != ("ddim",)
        self.row_coef = torch.zeros(tb.R, self.ROW_WIDTH if self._by_kind else 4, **f32)
        self.row_t, self.row_temb, self.row_kind = torch.zeros(tb.R, **f32), torch.zeros(tb.R, **i32), torch.zeros(tb.R, **i32)
        # the boundary's buffers: commands and fresh latents (two pinned stagings each, so the host can prepare one boundary
        # while the previous one's upload waits behind a replay), and the output ring with its pinned mirror
        self.cmd, self.fresh = torch.full((B, 4), -1, **i32), torch.zeros_like(self.lat)
        self.out = torch.zeros((self.out_capacity, c, s, s), **f32)
        self.out_host = torch.zeros((self.out_capacity, c, s, s), dtype=torch.float32, pin_memory=True)
        self._staging = [(torch.empty((B, 4), dtype=torch.int32, pin_memory=True),
                          torch.empty((B, c, s, s), dtype=torch.float32, pin_memory=True), torch.cuda.Event()) for _ in range(2)]
        self._upload(0, 0)
        self._model_key = model_state_key(unet)
        self._side, self._sync = [], [ops.new_sync_buffer(dev)]
        self.hist = self.noise = self.known = self.mask = self.filter = self._static = None
        if self._by_kind:
            # h1, h2 per slot.  Never cleared at a refill: a request's first row has b1 = b2 = 0 and its second b2 = 0, and the
            # update puts zeros in the place of a plane whose coefficient is 0, whatever the previous occupant left in it
            self.hist = torch.zeros((2,) + tuple(self.lat.shape), **f32)
        self._busy.clear()

    def _upload(self, row0, temb0):
        """Rows row0 .. and time-embedding rows temb0 .. of the host's record, written into the device tables in place."""
        tb = self.table
        if len(tb.t) > row0:
            dev = self.row_coef.device
            width = self.row_coef.shape[1]
            rows = [tuple(row) + (0.0,) * (width - len(row)) for row in tb.coef[row0:]]
            self.row_coef[row0:len(tb.t)].copy_(torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(dev))
            self.row_kind[row0:len(tb.t)].copy_(torch.tensor(tb.kind[row0:], dtype=torch.int32).to(dev))
            self.row_t[row0:len(tb.t)].copy_(torch.tensor(tb.t[row0:], dtype=torch.float32).to(dev))
            self.row_temb[row0:len(tb.t)].copy_(torch.tensor(tb.temb[row0:], dtype=torch.int32).to(dev))
        if len(tb.timesteps) > temb0:
            self.temb_table[temb0:len(tb.timesteps)].copy_(torch.cat([self.unet.temb_projection(t) for t in tb.timesteps[temb0:]], 0))

    def _retabulate(self):
        self._upload(len(self.table.t), 0)

    def add_schedule(self, schedule):
        """(begin, end): the schedule's rows in the row table, appended - with its unseen timesteps' projections - on the first
        call for this `schedule.key`."""
        rows, tembs = len(self.table.t), len(self.table.timesteps)
        span = self.table.add(schedule)
        self._upload(rows, tembs)
        return span

    def refresh_if_stale(self):
        """As the base class; the slots are emptied by a dtype or device change, so the model may only change between requests."""
        if self._busy and model_state_key(self.unet) != self._model_key:
            raise RuntimeError(f"SlotEngine: the model changed while {len(self._busy)} requests were in their slots")
        return super().refresh_if_stale()

    def _step(self):
        ops.slot_select(self.row_t, self.row_temb, self.pos, self.end, self.t_cur, self.active, self.temb_table, self.temb_rows)
        self._substep(self.lat, self.x_nhwc)

    def _apply(self, lat, eps, branch):
        if self._by_kind:
            ops.slot_step_kinds(lat, eps, self.hist, self.row_coef, self.row_kind, self.pos, self.active)
        else:
            ops.slot_step(lat, eps, self.row_coef, self.pos, self.active)

    def _carried(self):
        # (the history too: a capture happens with requests in their slots, and its warm-up step shifts their planes)
        return [self.lat, self.pos, self.t_cur, self.temb_rows, self.active] + ([] if self.hist is None else [self.hist])

    def _rewind(self):
        pass                        # (the cursors are carried: _capture puts them back)

    def reset(self, latents):
        raise NotImplementedError("SlotEngine has no schedule of its own: fill its slots with exchange()")

    run = reset

    def exchange(self, harvests, refills):
        """The boundary between replays.  harvests {slot: ring index}: the slot's latents go to out[index] and on to the pinned
        out_host[index]; refills {slot: (latents [C, H, W] or [1, C, H, W], already scaled, begin, end)}: the slot starts over on
        rows begin .. end - 1.  A slot in both is harvested first.  Returns {slot: event behind its device-to-host copy}.
        Nothing is launched when both are empty."""
        if not harvests and not refills:
            return {}
        for idx in harvests.values():
            if not 0 <= idx < self.out_capacity:
                raise ValueError(f"SlotEngine: output ring index {idx} of {self.out_capacity}")
        self._staging.append(self._staging.pop(0))
        cmd_host, fresh_host, uploaded = self._staging[-1]
        uploaded.synchronize()                        # (its previous upload: two boundaries ago)
        cmd = [[-1, -1, 0, 0] for _ in range(self.B)]
        on_device = []
        for i, (slot, (z, begin, end)) in enumerate(refills.items()):
            if not (0 <= begin <= end <= len(self.table.t)):
                raise ValueError(f"SlotEngine: rows {begin} .. {end} of {len(self.table.t)}")
            cmd[slot][1:] = [i, begin, end]
            z = z.reshape(self.lat.shape[1:])
            if z.device.type == "cpu":
                fresh_host[i].copy_(z)
            else:
                on_device.append((i, z))
        for slot, idx in harvests.items():
            cmd[slot][0] = idx
        cmd_host.copy_(torch.tensor(cmd, dtype=torch.int32))
        self.cmd.copy_(cmd_host, non_blocking=True)
        if len(refills) > len(on_device):
            self.fresh[:len(refills)].copy_(fresh_host[:len(refills)], non_blocking=True)
        uploaded.record()
        for i, z in on_device:
            self.fresh[i].copy_(z)
        ops.slot_exchange(self.cmd, self.lat, self.out, self.fresh, self.pos, self.end)
        self._busy.difference_update(harvests)
        self._busy.update(refills)
        events = {}
        for slot, idx in harvests.items():
            self.out_host[idx].copy_(self.out[idx], non_blocking=True)
            events[slot] = torch.cuda.Event()
            events[slot].record()
        return events

    def take(self, idx):
        """out_host[idx] as a tensor of its own [1, C, H, W]; the caller has waited for the harvest's event."""
        return self.out_host[idx].clone().unsqueeze(0)


class SeededSlotTable(SlotTable):
    """SlotTable for engines that also take "seeded" schedules: a third kind code and, per row, its ordinal - the row's place in
    its OWN schedule, 0 for the first evaluation, which is what the noise stream counts (not the row's index in the shared table)."""

    KIND_CODES = {"ddim": 0, "dpm": 1, "seeded": 2}        # what afldm_slot_step_seeded reads in row_kind

    def __init__(self, row_capacity, temb_capacity, kinds=("ddim", "seeded")):
        super().__init__(row_capacity, temb_capacity, kinds)
        self.ord = []                                      # per row: its ordinal

    def add(self, schedule):
        rows = len(self.t)
        span = super().add(schedule)                       # (raises before it appends: a refused schedule changes nothing)
        self.ord.extend(range(len(self.t) - rows))
        return span


class SeededSlotEngine(SlotEngine):
    """SlotEngine that takes stochastic requests: kind "seeded" (DDIMScheduler.seeded_schedule) next to "ddim" and, if asked for,
    "dpm".  The update is afldm_slot_step_seeded: afldm_slot_step_kinds plus the seeded update, whose noise is a function of the
    slot's seed, its row's ordinal (`row_ord`) and the element - so a request's result does not depend on the slot it sits in,
    on its neighbours or on the grouping into replays, and there is no noise feed.  exchange takes refills
    {slot: (latents, begin, end, seed)}; the seeds of all slots are uploaded at a refill from pinned staging (two buffers, each
    reused only after the event behind its previous upload, as the command buffer's)."""
    TABLE = SeededSlotTable

    def __init__(self, unet, batch_size, use_graph=True, steps_per_graph=5, *, row_capacity=1024, temb_capacity=256,
                 out_capacity=None, kinds=("ddim", "seeded")):
        super().__init__(unet, batch_size, use_graph, steps_per_graph, row_capacity=row_capacity, temb_capacity=temb_capacity,
                         out_capacity=out_capacity, kinds=kinds)

    def _allocate(self):
        dev = self.unet.device
        self.row_ord = torch.zeros(self.table.R, dtype=torch.int32, device=dev)      # (before the base class uploads the tables)
        self.seeds = torch.zeros(self.B, dtype=torch.int64, device=dev)
        self._seed_host = [0] * self.B                     # the host's mirror: every slot empty, as the base class leaves them
        self._seed_staging = [(torch.zeros(self.B, dtype=torch.int64, pin_memory=True), torch.cuda.Event()) for _ in range(2)]
        super()._allocate()

    def _upload(self, row0, temb0):
        super()._upload(row0, temb0)
        tb = self.table
        if len(tb.t) > row0:
            self.row_ord[row0:len(tb.t)].copy_(torch.tensor(tb.ord[row0:], dtype=torch.int32).to(self.row_ord.device))

    def _apply(self, lat, eps, branch):
        if not self._by_kind:
            return super()._apply(lat, eps, branch)
        ops.slot_step_seeded(lat, eps, self.hist, self.row_coef, self.row_kind, self.row_ord, self.pos, self.active, self.seeds)

    def exchange(self, harvests, refills):
        """As SlotEngine.exchange, with refills {slot: (latents, begin, end, seed)}: seed an integer in [0, 2^63), read by the
        slot's "seeded" rows only (a "ddim" or "dpm" request passes any, 0 say)."""
        plain, seeds = {}, {}
        for slot, refill in refills.items():
            if len(refill) != 4:
                raise ValueError("SeededSlotEngine: a refill is (latents, begin, end, seed)")
            seed = refill[3]
            if not (isinstance(seed, int) and not isinstance(seed, bool) and 0 <= seed < 2 ** 63):
                raise ValueError(f"SeededSlotEngine: seed {seed!r}, want an integer in [0, 2^63)")
            plain[slot], seeds[slot] = tuple(refill[:3]), seed
        events = super().exchange(harvests, plain)
        if seeds:
            for slot, seed in seeds.items():
                self._seed_host[slot] = seed
            self._seed_staging.append(self._seed_staging.pop(0))
            host, uploaded = self._seed_staging[-1]
            uploaded.synchronize()                    # (its previous upload: two refills ago)
            host.copy_(torch.tensor(self._seed_host, dtype=torch.int64))
            self.seeds.copy_(host, non_blocking=True)
            uploaded.record()
        return events


class EditSlotTable(SeededSlotTable):
    """SeededSlotTable for engines that also take the image-conditioned kinds: "seeded_sdedit" (img2img with a change map,
    DDIMScheduler.seeded_sdedit_schedule) and "seeded_repaint" (RePaint inpainting, DDIMScheduler.seeded_repaint_schedule).  A row's
    ordinal is its place in its own schedule, as in the parent - RePaint's schedule visits a timestep several times, and every
    visit has an ordinal, and so a noise, of its own."""

    KIND_CODES = {"ddim": 0, "dpm": 1, "seeded": 2, "seeded_sdedit": 3, "seeded_repaint": 4}      # what afldm_slot_step_edit reads

    def __init__(self, row_capacity, temb_capacity, kinds=("ddim", "seeded", "seeded_sdedit", "seeded_repaint")):
        super().__init__(row_capacity, temb_capacity, kinds)


class EditSlotEngine(SeededSlotEngine):
    """SeededSlotEngine that takes image-conditioned requests: kinds "seeded_sdedit" and "seeded_repaint" next to "ddim", "seeded"
    and, if asked for, "dpm".  The rows are 12 wide and the update is afldm_slot_step_edit: afldm_slot_step_seeded plus the two
    kinds, which read the slot's own conditioning planes - `cond` [B, C, S, S], its original or known latents, and `cmask`
    [B, 1, S, S], its change map or keep mask - and make all of their noise from the slot's seed and the row's ordinal.  So such a
    request's result, too, depends on nothing but the request.  exchange takes refills {slot: (latents, begin, end, seed, cond,
    cmask)}, cond and cmask None for the other kinds; the planes of a refilled slot are written on the engine's stream at the
    boundary - host tensors through pinned staging (two buffers, each reused only behind the event of its previous upload, as
    the fresh latents' and the seeds'), device tensors directly.  A slot's planes are only read by rows of the two kinds, so a
    request of another kind leaves whatever its predecessor put there."""
    TABLE = EditSlotTable
    ROW_WIDTH = 12
    PLANE_CODES = (EditSlotTable.KIND_CODES["seeded_sdedit"], EditSlotTable.KIND_CODES["seeded_repaint"])     # the kinds that read planes

    def __init__(self, unet, batch_size, use_graph=True, steps_per_graph=5, *, row_capacity=1024, temb_capacity=256,
                 out_capacity=None, kinds=("ddim", "seeded", "seeded_sdedit", "seeded_repaint")):
        super().__init__(unet, batch_size, use_graph, steps_per_graph, row_capacity=row_capacity, temb_capacity=temb_capacity,
                         out_capacity=out_capacity, kinds=kinds)

    def _allocate(self):
        unet, dev, B = self.unet, self.unet.device, self.B
        c, s = unet.config.in_channels, unet.config.sample_size
        self.cond = torch.zeros(B, c, s, s, dtype=torch.float32, device=dev)
        self.cmask = torch.zeros(B, 1, s, s, dtype=torch.float32, device=dev)
        self._plane_staging = [(torch.zeros(B, c, s, s, dtype=torch.float32, pin_memory=True),
                                torch.zeros(B, 1, s, s, dtype=torch.float32, pin_memory=True), torch.cuda.Event()) for _ in range(2)]
        super()._allocate()

    def _apply(self, lat, eps, branch):
        if not self._by_kind:
            return super()._apply(lat, eps, branch)
        ops.slot_step_edit(lat, eps, self.hist, self.cond, self.cmask, self.row_coef, self.row_kind, self.row_ord, self.pos,
                           self.active, self.seeds)

    def exchange(self, harvests, refills):
        """As SeededSlotEngine.exchange, with refills {slot: (latents, begin, end, seed, cond, cmask)}: cond [C, S, S] or
        [1, C, S, S] and cmask [S, S], [1, S, S] or [1, 1, S, S] for a request of an image-conditioned kind, (None, None) for any
        other; a span of such a kind without planes, and planes with any other span, raise.  A refill that is refused leaves the
        engine as it was."""
        seeded, planes = {}, {}
        for slot, refill in refills.items():
            if len(refill) != 6:
                raise ValueError("EditSlotEngine: a refill is (latents, begin, end, seed, cond, cmask)")
            cond, cmask = refill[4], refill[5]
            if (cond is None) != (cmask is None):
                raise ValueError("EditSlotEngine: a refill carries both planes, cond and cmask, or neither")
            begin, end = refill[1], refill[2]
            if 0 <= begin < end <= len(self.table.t):          # (any other span is the base class's to refuse)
                wants = self.table.kind[begin] in self.PLANE_CODES
                if wants != (cond is not None):
                    raise ValueError(f"EditSlotEngine: rows {begin} .. {end} are " + ("of an image-conditioned kind and need cond "
                                     "and cmask" if wants else "of a kind that reads no planes: pass None, None"))
            if cond is not None:
                if cond.numel() != self.cond[0].numel() or tuple(cond.shape[-3:]) != tuple(self.cond.shape[1:]):
                    raise ValueError(f"EditSlotEngine: cond {tuple(cond.shape)}, want {tuple(self.cond.shape[1:])}")
                if cmask.numel() != self.cmask[0].numel() or tuple(cmask.shape[-2:]) != tuple(self.cmask.shape[2:]):
                    raise ValueError(f"EditSlotEngine: cmask {tuple(cmask.shape)}, want {tuple(self.cmask.shape[1:])}")
                planes[slot] = (cond, cmask)
            seeded[slot] = tuple(refill[:4])
        events = super().exchange(harvests, seeded)
        if planes:
            cond_host = cmask_host = uploaded = None
            if any(t.device.type == "cpu" for pair in planes.values() for t in pair):
                self._plane_staging.append(self._plane_staging.pop(0))
                cond_host, cmask_host, uploaded = self._plane_staging[-1]
                uploaded.synchronize()                # (its previous upload: two such boundaries ago)
            for i, (slot, pair) in enumerate(planes.items()):
                for dst, host, t in ((self.cond[slot], cond_host, pair[0]), (self.cmask[slot], cmask_host, pair[1])):
                    t = t.reshape(dst.shape)
                    if t.device.type == "cpu":
                        host[i].copy_(t)
                        dst.copy_(host[i], non_blocking=True)
                    else:
                        dst.copy_(t)
            if uploaded is not None:
                uploaded.record()
        return events


class PicardEngine(DenoiseEngine):
    """Parallel-in-time sampling (ParaDiGMS, Shih et al., NeurIPS 2023) on the replayed graphs: every image keeps window + 1
    states X[0 .. window], estimates of window consecutive states of ONE "ddim" schedule, and an iteration evaluates the UNet on
    X[0 .. window - 1] of all P images as one batch of P window rows, sweeps the sampler's recurrence along the window with
    those outputs (afldm_picard_sweep), accepts the states whose predecessors moved by no more than `tolerance` in mean square
    (afldm_picard_stride: the stride s >= 1, the only place an image's cursor `base` moves, and the gather of the next
    evaluation's timesteps and time-embedding rows) and slides the window by s (afldm_picard_slide).  X[0] is always a state of
    the sequential sampler up to `tolerance`; with tolerance 0 it is that state exactly and the run is the plain DDIM sampler at
    batch P window, taking n iterations.  An image is finished when base == n; iterations replayed after that leave it alone.

    The states are state-major, [window + 1, P, C, S, S], so `lat` - rows 0 .. window - 1 - is the contiguous NCHW batch the
    plain step's layout conversion and UNet take unchanged (UNet row j P + p).  run() replays as many iterations as every
    unfinished image needs at the least, ceil((n - base) / window), then reads the cursors back - one small non-blocking copy
    into pinned memory and an event - and goes on until every image is finished.  stats: {"iterations", "evaluations"
    (iterations P window), "strides" (per iteration, one per image)}."""
    ONE_BRANCH = True           # one cursor table, one stride launch: no parallel branches

    def __init__(self, unet, scheduler, batch_size, num_inference_steps=50, use_graph=True, steps_per_graph=5, branches=1, *,
                 window=8, tolerance=0.1):
        kind = (scheduler if isinstance(scheduler, Schedule) else scheduler.schedule(num_inference_steps)).kind
        if kind not in self.UPDATES:
            raise NotImplementedError(f"PicardEngine: update_kind {kind!r}: the window takes 'ddim' schedules only (a stochastic kind "
                                      "needs a pre-drawn noise row per state, 'dpm' a history per state)")
        if unet.device.type != "cuda":
            raise RuntimeError("PicardEngine needs the UNet on an MI355X ('cuda') device; there is no CPU path")
        odd = sorted({type(m.processor).__name__ for m in unet.modules() if hasattr(m, "processor")} - {"AttnProcessor2_0"})
        if odd:
            raise ValueError(f"PicardEngine: the UNet has attention processors {odd}; the window needs the plain one")
        self.window, self.tolerance = self.check_window(window, tolerance)
        self.stats = None
        super().__init__(unet, scheduler, batch_size, num_inference_steps, use_graph, steps_per_graph, 1)

    @staticmethod
    def check_window(window, tolerance):
        """(window, tolerance) as the engine stores them; ValueError for a window below 1 (or above the kernels' 256) or a
        tolerance that is negative or NaN."""
        if int(window) != window or not 1 <= int(window) <= 256:
            raise ValueError(f"PicardEngine: window = {window} must be an integer in 1 .. 256")
        if not float(tolerance) >= 0.0:
            raise ValueError(f"PicardEngine: tolerance = {tolerance} must be >= 0")
        return int(window), float(tolerance)

    def _allocate(self):
        """Every device buffer in the UNet's current dtype and on its device; drops the graphs."""
        unet, dev, P, Wn, n = self.unet, self.unet.device, self.B, self.window, self.n
        c, s = unet.config.in_channels, unet.config.sample_size
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.states = torch.zeros(Wn + 1, P, c, s, s, **f32)
        self.lat = self.states[:Wn].view(Wn * P, c, s, s)          # what the UNet evaluates
        self.swept = torch.zeros(Wn, P, c, s, s, **f32)             # Y[1 .. Wn]
        self.partial = torch.zeros(P, Wn, ops.picard_blocks(c, s, s), **f32)
        self.x_nhwc = torch.empty(Wn * P, s, s, c, dtype=unet.dtype, device=dev)
        self.graph = self.graph_multi = None
        # per image: (base, iter) and the last stride; per (image, row): the last errors; per iteration: every image's stride
        self.cur, self.stride, self.err = torch.zeros(2, P, **i32), torch.zeros(P, **i32), torch.zeros(P, Wn, **f32)
        self.log = torch.zeros(n + self.steps_per_graph + 1, P, **i32)
        self.cur_host = torch.zeros(2, P, dtype=torch.int32, pin_memory=True)
        self._polled = torch.cuda.Event()
        # the row table, laid out as the slot sampler's: one time-embedding row per schedule row
        self.row_coef = self.schedule.table(dev).contiguous()
        self.row_t = torch.tensor(self.timesteps, dtype=torch.float32).to(dev)
        self.row_temb = torch.arange(n, **i32)
        self.temb_table = torch.cat([unet.temb_projection(t) for t in self.timesteps], 0).contiguous()
        self.t_cur, self.active = torch.zeros(Wn * P, **f32), torch.zeros(Wn * P, **i32)
        self.temb_rows = torch.zeros(Wn * P, self.temb_table.shape[1], dtype=unet.dtype, device=dev)   # (zeros: a row past the end evaluates finite)
        self.temb_slices = unet.temb_slices(self.temb_rows, per_sample=True)
        self._model_key = model_state_key(unet)
        self._side, self._sync = [], [ops.new_sync_buffer(dev)]
        self.hist = self.noise = self.known = self.mask = self.filter = self._static = None
        self._update, self._state = self.UPDATES[self.schedule.kind][0], [()]

    UPDATES = {"ddim": (ops.picard_sweep, DenoiseEngine._no_state)}

    def _gather(self, decide):
        ops.picard_stride(self.partial, self.cur, self.stride, self.err, self.log, self.row_t, self.row_temb, self.t_cur, self.active,
                          self.temb_table, self.temb_rows, self.tolerance ** 2, self.states.shape[2:], gather_only=not decide)

    def _step(self):
        self._substep(self.lat, self.x_nhwc)

    def _apply(self, lat, eps, branch):
        self._update(self.states, eps, self.swept, self.partial, self.row_coef, self.cur[0])
        self._gather(True)
        ops.picard_slide(self.states, self.swept, self.stride)

    def _carried(self):
        return [self.states, self.cur, self.stride, self.err, self.log, self.t_cur, self.active, self.temb_rows]

    def _rewind(self):
        pass                        # (the cursors are carried: _capture puts them back)

    def _result(self):
        return self.states[0].clone()

    def reset(self, latents):
        """latents [P, C, S, S]: every state of the window starts as the start latents, every cursor at row 0."""
        self.refresh_if_stale()
        self.states.copy_((latents.to(device=self.lat.device, dtype=torch.float32) * self.schedule.init_noise_sigma).unsqueeze(0)
                          .expand_as(self.states))
        self.cur.zero_()
        self.stride.zero_()
        self.log.zero_()
        self._gather(False)

    def _poll(self):
        """(base, iter) per image as they stand behind everything launched so far."""
        self.cur_host.copy_(self.cur, non_blocking=True)
        self._polled.record()
        self._polled.synchronize()
        return self.cur_host[0].tolist(), int(self.cur_host[1, 0])

    @torch.no_grad()
    def run(self, latents, draw=None, known=None):
        """latents [P, C, S, S] -> the sampled latents (fp32); `stats` says what it took.  draw and known do not apply."""
        if known is not None:
            raise ValueError("PicardEngine: known= goes with a 'repaint' or 'ilvr' schedule; the window takes 'ddim' ones")
        if tuple(latents.shape) != tuple(self.states.shape[1:]):
            raise ValueError(f"PicardEngine: latents {tuple(latents.shape)}, want {tuple(self.states.shape[1:])}")
        self.reset(latents)
        base, done = [0] * self.B, 0
        while min(base) < self.n:
            if done >= self.n:
                raise RuntimeError(f"PicardEngine: {done} iterations of a {self.n}-row schedule and the cursors stand at {base}: "
                                   "every iteration advances an unfinished image by one row at the least")
            # what every unfinished image needs at the least, within what is left of the n iterations that always suffice
            self.step(min(max(-(-(self.n - b) // self.window) for b in base), self.n - done))
            base, done = self._poll()
        out = self._result()
        strides = self.log[:done].tolist()
        while strides and not any(strides[-1]):
            strides.pop()           # (iterations of a replay group after the last image finished)
        self.stats = {"iterations": len(strides), "evaluations": len(strides) * self.B * self.window, "strides": strides}
        self.check_errors()
        return out
