"""Image-conditioned requests in slots, the host side (no GPU): the two schedules against their generator-driven twins,
EditSlotTable, the header / library / binding of afldm_slot_step_edit, the float32 restatement of tests/edit_oracle.py against the
float64 formulas, and SamplingServer's edit requests against a counting engine."""
import math
import types

import numpy as np
import pytest
import torch

import edit_oracle as eo
import noise_oracle as no
from test_counter_noise_host import SeededCountingEngine

EDIT_KINDS = ("ddim", "dpm", "seeded", "seeded_sdedit", "seeded_repaint")


def _ddim():
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    return ffhq_ddim_scheduler()


def _dpm():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, solver_order=2)


# ------------------------------------------------------------------------------------------------ 1. the schedules
def test_the_two_schedules_are_their_twins_without_draws():
    from afldm_amd.schedulers.schedule import KINDS, NOISE_SLOTS, ROW_WIDTH
    assert KINDS["seeded_sdedit"] == (12, 2, False) and KINDS["seeded_repaint"] == (12, 3, False)
    assert ROW_WIDTH["seeded_sdedit"] == ROW_WIDTH["seeded_repaint"] == 12
    assert "seeded_sdedit" not in NOISE_SLOTS and "seeded_repaint" not in NOISE_SLOTS
    keys = set()
    for n, strength, eta in ((50, 0.3, 0.0), (6, 1.0, 0.7), (10, 0.55, 1.0)):
        twin, got = _ddim().sdedit_schedule(n, strength, eta), _ddim().seeded_sdedit_schedule(n, strength, eta)
        assert got.kind == "seeded_sdedit" and twin.kind == "sdedit" and len(got.rows) == min(int(n * strength), n)
        assert got.rows == twin.rows and got.timesteps == twin.timesteps and got.init_noise_sigma == twin.init_noise_sigma
        assert got.draws == ((False, False),) * len(got.rows) and [got.slots(k) for k in range(len(got.rows))] == [()] * len(got.rows)
        assert got.key != twin.key and got.key == _ddim().seeded_sdedit_schedule(n, strength, eta).key
        keys |= {got.key, twin.key}
    assert len(_ddim().seeded_sdedit_schedule(50, 0.3).rows) == 15
    for n, eta, jl, js in ((6, 0.0, 2, 2), (20, 0.5, 5, 2), (7, 1.0, 3, 3)):
        twin, got = _ddim().repaint_schedule(n, eta, jl, js), _ddim().seeded_repaint_schedule(n, eta, jl, js)
        assert got.kind == "seeded_repaint" and twin.kind == "repaint"
        assert got.rows == twin.rows and got.timesteps == twin.timesteps and got.init_noise_sigma == twin.init_noise_sigma
        assert got.draws == ((False, False, False),) * len(got.rows) and any(any(d) for d in twin.draws)
        assert [got.slots(k) for k in range(len(got.rows))] == [()] * len(got.rows)
        assert got.key != twin.key and got.key == _ddim().seeded_repaint_schedule(n, eta, jl, js).key
        keys |= {got.key, twin.key}
    assert len(keys) == 12
    rp = _ddim().seeded_repaint_schedule(6, 0.0, 2, 2)
    assert len(rp.rows) == 10 and len(set(rp.timesteps)) == 6, "RePaint visits timesteps more than once"
    assert _ddim().seeded_repaint_schedule(6, 0.0, 2, 2).key != _ddim().seeded_repaint_schedule(6, 0.0, 2, 3).key
    assert _ddim().seeded_sdedit_schedule(10, 0.5).key != _ddim().seeded_sdedit_schedule(10, 0.6).key
    with pytest.raises(ValueError, match="strength"):
        _ddim().seeded_sdedit_schedule(10, 0.05)
    with pytest.raises(ValueError, match="jump"):
        _ddim().seeded_repaint_schedule(10, 0.0, 0, 1)
    # a kind of several slots may still not draw where the kind says so
    from afldm_amd.schedulers.schedule import Schedule
    with pytest.raises(AssertionError):
        Schedule.of(_ddim(), "seeded_repaint", rp.timesteps, rp.rows, [(True, False, False)] * 10, _probe=1)


# ------------------------------------------------------------------------------------------------ 2. the table
def test_edit_table_codes_and_ordinals():
    from afldm_amd.engine import EditSlotTable, SeededSlotTable, SlotTable
    assert SlotTable.KIND_CODES == {"ddim": 0, "dpm": 1}
    assert SeededSlotTable.KIND_CODES == {"ddim": 0, "dpm": 1, "seeded": 2}
    assert EditSlotTable.KIND_CODES == {"ddim": 0, "dpm": 1, "seeded": 2, "seeded_sdedit": 3, "seeded_repaint": 4}
    tb = EditSlotTable(64, 48, kinds=EDIT_KINDS)
    d3, e4, p2 = _ddim().schedule(3), _ddim().seeded_sdedit_schedule(8, 0.5, 0.3), _dpm().schedule(2)
    r10, s2 = _ddim().seeded_repaint_schedule(6, 0.0, 2, 2), _ddim().seeded_schedule(2, 0.5)
    assert tb.add(d3) == (0, 3) and tb.add(e4) == (3, 7) and tb.add(p2) == (7, 9) and tb.add(r10) == (9, 19) and tb.add(s2) == (19, 21)
    assert tb.kind == [0] * 3 + [3] * 4 + [1] * 2 + [4] * 10 + [2] * 2
    # a row's ordinal is its place in its OWN schedule: RePaint's repeated timesteps each have one of their own
    assert tb.ord == [0, 1, 2] + [0, 1, 2, 3] + [0, 1] + list(range(10)) + [0, 1]
    assert tb.t[9:19] == [float(t) for t in r10.timesteps] and len(set(tb.temb[9:19])) == 6
    assert tb.coef[3:7] == list(e4.rows) and tb.coef[9:19] == list(r10.rows) and all(len(r) == 12 for r in tb.coef[3:7] + tb.coef[9:19])
    assert tb.add(_ddim().seeded_repaint_schedule(6, 0.0, 2, 2)) == (9, 19) and len(tb.ord) == len(tb.t) == 21
    assert EditSlotTable(8, 8).kinds == ("ddim", "seeded", "seeded_sdedit", "seeded_repaint")
    with pytest.raises(ValueError, match="kinds"):
        EditSlotTable(8, 8, kinds=("ddim", "sdedit"))
    with pytest.raises(ValueError, match="kinds"):
        SeededSlotTable(8, 8, kinds=("ddim", "seeded_sdedit"))
    with pytest.raises(ValueError, match="kinds"):
        SlotTable(8, 8, kinds=("ddim", "seeded_repaint"))


def test_a_refused_schedule_leaves_the_edit_table_unchanged():
    from afldm_amd.engine import EditSlotTable, SeededSlotTable
    tb = EditSlotTable(12, 32)
    tb.add(_ddim().seeded_repaint_schedule(6, 0.0, 2, 2))

    def state():
        return (list(tb.coef), list(tb.kind), list(tb.ord), list(tb.t), list(tb.temb), list(tb.timesteps), dict(tb.spans))
    before = state()
    with pytest.raises(RuntimeError, match="row table is full"):
        tb.add(_ddim().seeded_sdedit_schedule(6, 0.5))
    for refused in (_dpm().schedule(2), _ddim().sdedit_schedule(6, 0.5), _ddim().repaint_schedule(6, 0.0, 2, 2),
                    _ddim().stochastic_schedule(2, 0.5)):
        with pytest.raises(NotImplementedError, match="schedules only"):
            tb.add(refused)
    assert state() == before and tb.ord == list(range(10))
    seeded = SeededSlotTable(32, 32)
    for refused in (_ddim().seeded_sdedit_schedule(6, 0.5), _ddim().seeded_repaint_schedule(6, 0.0, 2, 2)):
        with pytest.raises(NotImplementedError, match="schedules only"):
            seeded.add(refused)
    assert not seeded.t and not seeded.ord


# ------------------------------------------------------------------------------------------------ 3. the binding
def test_the_edit_entry_point_is_declared_built_and_bound():
    import os
    import re
    import subprocess
    import sys
    from afldm_amd import _edit, _lib, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "afldm_hip_edit.h")).read()
    declared = set(re.findall(r"^int\s+(afldm_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert declared == {"afldm_slot_step_edit"} == set(_edit.exports()) == set(_lib.EDIT_ABI.functions)
    nm = subprocess.run(["nm", "-D", "--defined-only", _edit.EDIT_PATH], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if " T afldm_" in l} == declared
    assert not declared & set(_lib.EXPORTS) and not declared & set(_lib.SLOTS_ABI.functions) and not declared & set(_lib.NOISE_ABI.functions)
    assert build.EDIT_SOURCES == ["edit.hip"] and build.EDIT_LIB.endswith("libafldm_edit.so") and callable(ops.slot_step_edit)
    assert len(_edit.lib().afldm_slot_step_edit.argtypes) == 18
    assert "afldm_slot_step_edit" in open(os.path.join(root, "INTEGRATION.md")).read()
    # refusals before any launch: NULL pointers, bad shapes
    lib = _edit.lib()
    assert lib.afldm_slot_step_edit(*([None] * 11), 1, 1, 1, 1, 1, 0, None) == -5
    assert lib.afldm_slot_step_edit(*([16] * 10), None, 1, 1, 1, 1, 1, 0, None) == -5
    for shape in ((0, 1, 1, 1, 1), (65536, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0),
                  (1, 1, 1 << 11, 1 << 10, 1 << 10)):
        assert lib.afldm_slot_step_edit(*([16] * 11), *shape, 0, None) == -1, shape
    assert b"afldm_slot_step_edit" in _lib.lib.afldm_last_error()
    code = ("import sys; sys.path.insert(0, %r); import afldm_amd, afldm_amd.ops, afldm_amd.engine, afldm_amd.serving; "
            "import afldm_amd.models.unet_2d; print(any('libafldm_edit' in l for l in open('/proc/self/maps')))" % root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert r.stdout.strip().splitlines()[-1] == "False", r.stdout


# ------------------------------------------------------------------------------------------------ 4. the restatement
def test_the_float32_restatements_follow_the_formulas():
    """The oracle's float32 restatements against the float64 formulas - on made-up rows with an active clamp and on every row of the
    product's two schedules - and its noise slots against the kinds' (KINDS)."""
    from afldm_amd.schedulers.schedule import KINDS
    assert {len(eo.NOISE_SLOTS[eo.KIND_SDEDIT]), len(eo.NOISE_SLOTS[eo.KIND_REPAINT])} == {KINDS["seeded_sdedit"][1], KINDS["seeded_repaint"][1]}
    g = np.random.default_rng(5)
    x, e, o, zk, zu, zb = (g.standard_normal(64).astype(np.float32) for _ in range(6))
    m = g.uniform(0, 1, 64).astype(np.float32)
    t64 = [torch.from_numpy(v).double() for v in (x, e, o, m, zk, zu, zb)]
    sd_row = (1.2, -0.6, -0.8, 0.7, 0.85, 0.35, 0.45, 0.9, 0.4, 0.5, 0.0, 0.0)
    got = eo.sdedit32(x, e, o, m, zk, zu, sd_row)
    ref = eo.sdedit64(t64[0], t64[1], t64[2], t64[3], t64[4], t64[5], sd_row).numpy()
    assert np.abs(got - ref).max() <= 1e-5 and (m <= 0.5).any() and (m > 0.5).any()
    rp_row = (1.2, -0.6, -0.8, 0.7, 0.85, 0.35, 0.45, 0.9, 0.4, 0.95, 0.3, 0.0)
    got = eo.repaint32(x, e, o, m, zk, zu, zb, rp_row)
    ref = eo.repaint64(*t64, rp_row).numpy()
    assert np.abs(got - ref).max() <= 1e-5
    for row in _ddim().seeded_sdedit_schedule(8, 0.5, 0.7).rows:
        got = eo.sdedit32(x, e, o, m, zk, zu, row)
        assert np.abs(got - eo.sdedit64(t64[0], t64[1], t64[2], t64[3], t64[4], t64[5], row).numpy()).max() <= 1e-4
    for row in _ddim().seeded_repaint_schedule(6, 0.7, 2, 2).rows:
        assert np.abs(eo.repaint32(x, e, o, m, zk, zu, zb, row) - eo.repaint64(*t64, row).numpy()).max() <= 1e-4
    # the select: a held element takes nothing of x, e or z_u; a NaN in the map compares false and generates the element
    xn, en, mn = x.copy(), e.copy(), m.copy()
    held = m <= 0.5
    xn[held], en[held] = np.nan, np.inf
    mn[~held] = np.nan
    out = eo.sdedit32(xn, en, o, mn, zk, zu, sd_row)
    plain = eo.sdedit32(x, e, o, m, zk, zu, sd_row)
    assert np.array_equal(out, plain) and np.isfinite(out).all()
    # a product rounded on its own, not fused: p x + q e with p x inexact
    one = eo.sdedit32(np.float32(1 + 2 ** -23), np.float32(1.0), 0, 1.0, 0, 0, (1 + 2 ** -23, -1.0, -math.inf, math.inf, 1.0, 0, 0, 0, 0, 0.5))
    assert float(one) == float(np.float32(np.float32(1 + 2 ** -23) * np.float32(1 + 2 ** -23)) - np.float32(1.0))
    # slot_step: the stream slots and ordinals of each noise
    asked = []

    def noise(seed, ordinal, slot):
        asked.append((seed, ordinal, slot))
        return no.normals(seed, ordinal, 8, slot, np.float32).reshape(2, 2, 2)
    rows = np.array([sd_row, rp_row, (1, 0, -math.inf, math.inf, 1, 0, 0, 1, 0, 0.5, 0, 0)], dtype=np.float64)
    xs = g.standard_normal((4, 2, 2, 2)).astype(np.float32)
    out = eo.slot_step(xs, xs, xs, np.full((4, 1, 2, 2), 0.25, np.float32), rows, [3, 4, 3], [7, 9, 11], [0, 1, 2, 1], [1, 1, 1, 0],
                       [21, 22, 23, 24], noise)
    assert asked == [(21, 7, 0), (21, 0, 1), (22, 9, 0), (22, 9, 1), (22, 9, 2)], "slot 2's row has c = k1 = 0; slot 3 is inactive"
    assert np.array_equal(out[3], xs[3]) and not np.array_equal(out[0], xs[0])


# ------------------------------------------------------------------------------------------------ 5. the server
class EditCountingEngine(SeededCountingEngine):
    """The counting engine with an EditSlotTable; refills are (latents, begin, end, seed, cond, cmask) and every one is recorded."""

    def __init__(self, B, steps_per_graph, kinds, **kw):
        from afldm_amd.engine import EditSlotTable
        super().__init__(B, steps_per_graph, kinds=("ddim", "seeded"), **kw)
        self.table = EditSlotTable(self.table.R, self.table.T, kinds=kinds)
        self.planes = []

    def exchange(self, harvests, refills):
        for b, refill in refills.items():
            assert len(refill) == 6
            self.planes.append((float(refill[0].reshape(-1)[0]), refill[4], refill[5]))
        return super().exchange(harvests, {b: r[:4] for b, r in refills.items()})


def _pipe(scheduler=None):
    unet = types.SimpleNamespace(config=types.SimpleNamespace(in_channels=2, sample_size=1), device=torch.device("cpu"),
                                 dtype=torch.float32)
    return types.SimpleNamespace(unet=unet, scheduler=scheduler or _ddim())


@pytest.fixture
def host_ops(monkeypatch):
    """ops.counter_noise and ops.sdedit_step_flat restated on the host (the stream of noise_oracle, held = k0 orig + k1 z), so
    that submit_img2img_latents runs without a GPU; records the (seed, ordinal, slot) asked for."""
    from afldm_amd import ops
    asked = []

    def counter_noise(seeds, ordinals, shape, slot=0, out=None):
        asked.append((seeds.tolist(), ordinals.tolist(), tuple(shape), slot))
        return torch.from_numpy(no.noise(seeds.tolist(), ordinals.tolist(), tuple(shape), slot, np.float32))

    def sdedit_step_flat(x, eps, orig, cmap, z, z_u, row, out=None):
        assert z_u is None and tuple(row[:7]) == (0.0, 0.0, -math.inf, math.inf, 0.0, 0.0, 0.0) and row[9] == math.inf
        assert not x.any() and not eps.any() and not cmap.any()
        return torch.from_numpy(eo.sdedit32(x.numpy(), eps.numpy(), orig.numpy(), cmap.numpy(), z.numpy(), 0 * z.numpy(), row))
    monkeypatch.setattr(ops, "counter_noise", counter_noise)
    monkeypatch.setattr(ops, "sdedit_step_flat", sdedit_step_flat)
    return asked


def _server(slots, steps_per_graph, kinds=EDIT_KINDS, pipe=None):
    from afldm_amd.serving import SamplingServer
    return SamplingServer(pipe or _pipe(), slots, steps_per_graph, kinds=kinds,
                          engine_factory=lambda i: EditCountingEngine(slots, steps_per_graph, kinds))


def _lat(v):
    return torch.tensor([float(v), 0.0]).reshape(1, 2, 1, 1)


@pytest.mark.parametrize("steps_per_graph", [1, 3])
def test_planes_travel_with_the_refills_of_edit_requests(steps_per_graph, host_ops):
    from afldm_amd.utils import randn_tensor
    server = _server(2, steps_per_graph)
    eng = server.engines[0]
    cmap, mask = torch.full((1, 1, 1, 1), 0.5), torch.ones(1, 1, 1, 1)
    tickets = [server.submit(3, latents=_lat(1000)),
               server.submit_img2img_latents(_lat(2000), strength=0.5, change_map=cmap, num_inference_steps=8, eta=0.3, seed=41),
               server.submit_inpaint_latents(_lat(3000), mask, num_inference_steps=6, jump_length=2, jump_n_sample=2, seed=42),
               server.submit(4, eta=0.5, seed=43, latents=_lat(4000)),
               server.submit_img2img_latents(_lat(5000), strength=0.3, num_inference_steps=50, seed=44),
               server.submit(2, solver="dpm", latents=_lat(6000))]
    assert host_ops == [([41], [0], (1, 2, 1, 1), 1), ([44], [0], (1, 2, 1, 1), 1)], "the fixed noise: slot 1 at ordinal 0"
    assert [t.steps for t in tickets] == [3, 4, 10, 4, 15, 2]
    assert [eng.table.kind[t._span[0]] for t in tickets] == [0, 3, 4, 2, 3, 1]
    # the starts: k0_start orig + k1_start z for img2img, the seed's draw for inpainting
    k0s, k1s = _ddim().sdedit_start(8, 0.5)
    z = no.normals(41, 0, 2, 1, np.float32)
    want = np.float32(np.float32(k0s) * np.float32(2000.0)) + np.float32(np.float32(k1s) * z[0])
    assert float(tickets[1]._start.reshape(-1)[0]) == float(want)
    assert torch.equal(tickets[2]._start, randn_tensor((1, 2, 1, 1), generator=torch.Generator().manual_seed(42)))
    starts = [float(t._start.reshape(-1)[0]) for t in tickets]
    while server.poll(max_replays=1):
        mirror = [0 if s is None else s[1] for s in server._slot[0]]
        assert mirror == eng.remaining(), (mirror, eng.remaining())
    server.run()
    for ticket, start in zip(tickets, starts):
        assert float(ticket.result()[0, 0]) == pytest.approx(start + ticket.steps), "one evaluation per row of its schedule"
        assert eng.table.ord[ticket._span[0]:ticket._span[1]] == list(range(ticket.steps))
    assert server.useful == sum(t.steps for t in tickets) == 38
    # every refill in arrival order: planes for the edit requests, None for the others
    assert [p[0] for p in eng.planes] == starts
    conds = [None, 2000.0, 3000.0, None, 5000.0, None]
    for (_, cond, cmask), want in zip(eng.planes, conds):
        if want is None:
            assert cond is None and cmask is None
        else:
            assert cond.dtype == cmask.dtype == torch.float32 and tuple(cond.shape) == (1, 2, 1, 1) and tuple(cmask.shape) == (1, 1, 1, 1)
            assert float(cond.reshape(-1)[0]) == want
    assert float(eng.planes[1][2]) == 0.5 and float(eng.planes[2][2]) == 1.0 and float(eng.planes[4][2]) == 1.0, "no map: all ones"
    assert eng.seen == [(s, seed) for s, seed in zip(starts, (0, 41, 42, 43, 44, 0))]
    assert all(t._planes == (None, None) and t._composite is None for t in tickets), "a ticket hands its planes over with the refill"


def test_edit_requests_need_a_seed_planes_of_the_right_shape_and_an_edit_server(host_ops):
    from afldm_amd.serving import SamplingServer
    from test_slots_dpm_host import KindsCountingEngine
    server = _server(2, 2)
    mask = torch.ones(1, 1, 1, 1)
    for bad in (None, -1, 2 ** 63, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            server.submit_img2img_latents(_lat(1), seed=bad)
        with pytest.raises(ValueError, match="seed"):
            server.submit_inpaint_latents(_lat(1), mask, seed=bad)
    with pytest.raises(ValueError, match="orig_latents"):
        server.submit_img2img_latents(torch.zeros(2, 2, 1, 1), seed=1)
    with pytest.raises(ValueError, match="change_map"):
        server.submit_img2img_latents(_lat(1), change_map=torch.zeros(1, 2, 1, 1), seed=1)
    with pytest.raises(ValueError, match="known_latents"):
        server.submit_inpaint_latents(torch.zeros(1, 2, 2, 1), mask, seed=1)
    with pytest.raises(ValueError, match="latent_mask"):
        server.submit_inpaint_latents(_lat(1), torch.ones(1, 1, 2, 2), seed=1)
    with pytest.raises(ValueError, match="strength"):
        server.submit_img2img_latents(_lat(1), strength=0.01, seed=1)          # no evaluation: img2img_latents' own refusal
    with pytest.raises(ValueError, match="submit_img2img_latents"):
        server.submit(schedule=_ddim().seeded_sdedit_schedule(6, 0.5), seed=1)
    assert not server._queue[0] and server._count == 0 and not server.engines[0].table.t
    # servers without the edit kinds: the engine's refusal, nothing queued, and their refills stay as they were
    for kinds, cls in ((("ddim",), KindsCountingEngine), (("ddim", "dpm"), KindsCountingEngine)):
        plain = SamplingServer(_pipe(), 2, 2, kinds=kinds, engine_factory=lambda i: cls(2, 2, kinds))
        with pytest.raises(NotImplementedError, match="schedules only"):
            plain.submit_img2img_latents(_lat(1), seed=1)
        with pytest.raises(NotImplementedError, match="schedules only"):
            plain.submit_inpaint_latents(_lat(1), mask, num_inference_steps=6, seed=1)
        assert not plain._queue[0] and plain._count == 0
        t = plain.submit(2, latents=_lat(0))
        plain.run()
        assert float(t.result()[0, 0]) == 2
    seeded = SamplingServer(_pipe(), 2, 2, kinds=("ddim", "seeded"),
                            engine_factory=lambda i: SeededCountingEngine(2, 2, ("ddim", "seeded")))
    with pytest.raises(NotImplementedError, match="schedules only"):
        seeded.submit_inpaint_latents(_lat(1), mask, num_inference_steps=6, seed=1)
    t = seeded.submit(2, eta=0.5, seed=3, latents=_lat(0))
    seeded.run()
    assert float(t.result()[0, 0]) == 2 and seeded._seeded and not seeded._edit
    # a DPM pipeline's edit requests are DDIM ones of its noise schedule
    dpm_server = _server(2, 2, pipe=_pipe(_dpm()))
    t = dpm_server.submit_inpaint_latents(_lat(1), mask, num_inference_steps=6, jump_length=2, jump_n_sample=2, seed=9)
    assert t.steps == 10 and dpm_server.engines[0].table.kind[t._span[0]] == 4
