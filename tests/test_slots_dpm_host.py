"""DPM-Solver++ requests in slots, the host side without a GPU: SlotTable with kinds=("ddim", "dpm") (afldm_amd/engine.py),
SamplingServer on a pipeline whose scheduler is a DPMSolverMultistepScheduler (afldm_amd/serving.py) against the counting
engine of tests/test_slots_host.py, and tests/slot_dpm_oracle.py's sampler against the restated solver of
tests/test_dpm_host.py."""
import types

import pytest
import torch

import slot_dpm_oracle as sdo
from test_dpm_host import RefSolver, ref_sigmas, ref_timesteps
from test_slots_host import CountingEngine

KINDS = ("ddim", "dpm")


def _dpm(order=2):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, solver_order=order)


def _ddim():
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    return ffhq_ddim_scheduler()


# ------------------------------------------------------------------------------------------------ 1. the table
def test_table_holds_both_kinds_and_shares_timestep_rows():
    from afldm_amd.engine import SlotTable
    tb = SlotTable(64, 48, kinds=KINDS)
    d5, p4, p9 = _ddim().schedule(5), _dpm(2).schedule(4), _dpm(3).schedule(9)
    assert tb.add(d5) == (0, 5) and tb.add(p4) == (5, 9) and tb.add(p9) == (9, 18)
    assert tb.spans == {d5.key: (0, 5), p4.key: (5, 9), p9.key: (9, 18)}
    assert tb.kind == [0] * 5 + [1] * 13 and SlotTable.KIND_CODES == {"ddim": 0, "dpm": 1}
    assert tb.coef == list(d5.rows + p4.rows + p9.rows)                       # the schedules' own tuples: 4 wide, then 8 wide
    assert [len(r) for r in tb.coef] == [4] * 5 + [8] * 13
    assert tb.t == [float(t) for t in d5.timesteps + p4.timesteps + p9.timesteps]
    # one time-embedding row per distinct timestep, whichever kind asked for it first
    distinct = set(d5.timesteps) | set(p4.timesteps) | set(p9.timesteps)
    assert len(tb.timesteps) == len(set(tb.timesteps)) == len(distinct) < 18
    assert [tb.timesteps[i] for i in tb.temb] == list(d5.timesteps + p4.timesteps + p9.timesteps)
    # (FFHQ config, "leading" spacing: DDIM 5 evaluates at 801 .. 1, DPM 4 at 801 .. 201)
    assert set(p4.timesteps) < set(d5.timesteps)
    for t in p4.timesteps:
        assert tb.temb[d5.timesteps.index(t)] == tb.temb[5 + p4.timesteps.index(t)]
    # the same schedule again: the same span, nothing appended
    assert tb.add(_dpm(2).schedule(4)) == (5, 9) and tb.add(_ddim().schedule(5)) == (0, 5) and len(tb.t) == 18
    # the rows' zero pattern is what keeps a stale history out: first row b1 = b2 = 0, second b2 = 0
    first, second, third = p9.rows[0], p9.rows[1], p9.rows[2]
    assert first[4] == 0.0 and first[5] == 0.0 and second[4] != 0.0 and second[5] == 0.0 and third[4] != 0.0 and third[5] != 0.0


def test_a_full_table_is_left_unchanged():
    from afldm_amd.engine import SlotTable
    tb = SlotTable(7, 32, kinds=KINDS)
    tb.add(_dpm().schedule(5))
    before = (list(tb.coef), list(tb.kind), list(tb.t), list(tb.temb), list(tb.timesteps), dict(tb.spans))
    with pytest.raises(RuntimeError, match="row table is full"):
        tb.add(_ddim().schedule(3))
    with pytest.raises(RuntimeError, match="row table is full"):
        tb.add(_dpm().schedule(3))
    assert (tb.coef, tb.kind, tb.t, tb.temb, tb.timesteps, tb.spans) == before


def test_refusals():
    from afldm_amd.engine import SlotTable
    default = SlotTable(64, 32)
    assert default.kinds == ("ddim",)
    with pytest.raises(NotImplementedError, match="'ddim' schedules only"):
        default.add(_dpm().schedule(5))
    assert not default.t and not default.kind and not default.spans
    both = SlotTable(64, 32, kinds=KINDS)
    with pytest.raises(NotImplementedError, match="'ddim' schedules only") as info:
        both.add(_ddim().stochastic_schedule(5, 0.5))
    assert "'dpm'" in str(info.value) and "'sde'" in str(info.value)
    assert not both.t and not both.spans
    for bad in (("ddim", "sde"), ("dpm", "euler"), ()):
        with pytest.raises(ValueError, match="kinds"):
            SlotTable(64, 32, kinds=bad)


# ------------------------------------------------------------------------------------------------ 2. the server
class KindsCountingEngine(CountingEngine):
    def __init__(self, B, steps_per_graph, kinds, **kw):
        from afldm_amd.engine import SlotTable
        super().__init__(B, steps_per_graph, **kw)
        self.table = SlotTable(self.table.R, self.table.T, kinds=kinds)


def _pipe(scheduler):
    unet = types.SimpleNamespace(config=types.SimpleNamespace(in_channels=2, sample_size=1), device=torch.device("cpu"),
                                 dtype=torch.float32)
    return types.SimpleNamespace(unet=unet, scheduler=scheduler)


def _server(scheduler, slots, steps_per_graph, kinds=None):
    from afldm_amd.serving import SamplingServer
    pipe = _pipe(scheduler)
    table_kinds = SamplingServer.default_kinds(pipe) if kinds is None else kinds          # (what the server hands a SlotEngine)
    return SamplingServer(pipe, slots, steps_per_graph, kinds=kinds,
                          engine_factory=lambda i: KindsCountingEngine(slots, steps_per_graph, table_kinds))


SOLVERS = (None, "ddim", "dpm", "dpm", None, "ddim", "dpm", "ddim", None, "dpm", "ddim")
LENGTHS = (3, 5, 2, 4, 16, 5, 1, 2, 5, 4, 3)


@pytest.mark.parametrize("steps_per_graph", [1, 2, 3])
def test_mixed_solvers_on_a_dpm_pipe_keep_the_mirror_exact(steps_per_graph):
    server = _server(_dpm(), 4, steps_per_graph)
    assert server.kinds == KINDS
    eng = server.engines[0]
    tickets = [server.submit(n, latents=torch.tensor([1000.0 * i, 0.0]).reshape(1, 2, 1, 1), solver=s)
               for i, (n, s) in enumerate(zip(LENGTHS, SOLVERS))]
    while server.poll(max_replays=1):
        mirror = [0 if s is None else s[1] for s in server._slot[0]]
        assert mirror == eng.remaining(), (mirror, eng.remaining())
    server.run()
    for i, (ticket, n, s) in enumerate(zip(tickets, LENGTHS, SOLVERS)):
        got = ticket.result()
        want = server._schedule(n, s)
        assert want.kind == ("ddim" if s == "ddim" else "dpm") and len(want.timesteps) == n
        assert float(got[0, 0]) == 1000.0 * i + n and float(got[0, 1]) == float(sum(want.timesteps)), (i, n, s)
    assert server.useful == sum(LENGTHS) and server.replays == eng.replays
    # both kinds sit in one table, each (solver, step count) once
    kinds = [eng.table.kind[b] for b, _ in sorted(eng.table.spans.values())]
    assert set(kinds) == {0, 1} and len(eng.table.spans) == len({(n, "ddim" if s == "ddim" else "dpm") for n, s in zip(LENGTHS, SOLVERS)})


def test_schedule_of_a_dpm_pipe_is_a_fresh_dpm_schedule():
    pipe_sched = _dpm(3)
    pipe_sched.set_timesteps(7)
    server = _server(pipe_sched, 2, 2)
    for n in (5, 16):
        s = server._schedule(n)
        assert s.kind == "dpm" and len(s.rows) == len(s.timesteps) == n and all(len(r) == 8 for r in s.rows)
        assert s.key == _dpm(3).schedule(n).key and s.rows == _dpm(3).schedule(n).rows
    assert pipe_sched.num_inference_steps == 7                        # the pipeline's own scheduler is left alone
    assert server._schedule(4, "ddim").kind == "ddim" and server._schedule(4, "dpm").kind == "dpm"
    with pytest.raises(ValueError, match="solver"):
        server.submit(3, solver="euler")


def test_default_kinds_follow_the_pipe_scheduler_and_a_missing_kind_is_refused():
    from afldm_amd.serving import SamplingServer
    assert SamplingServer.default_kinds(_pipe(_ddim())) == ("ddim",) and SamplingServer.default_kinds(_pipe(_dpm())) == KINDS
    server = _server(_ddim(), 2, 2)
    assert server.kinds == ("ddim",) and server._schedule(3).kind == "ddim"
    with pytest.raises(NotImplementedError, match="'ddim' schedules only"):
        server.submit(3, solver="dpm")
    with pytest.raises(NotImplementedError, match="'ddim' schedules only"):
        server.submit(schedule=_dpm().schedule(3))
    assert not server._queue[0] and server._count == 0
    # opted in on a DDIM pipe: DDIM by default, DPM per request, built from the DDIM config
    server = _server(_ddim(), 2, 2, kinds=KINDS)
    a, b = server.submit(3, latents=torch.zeros(1, 2, 1, 1)), server.submit(4, latents=torch.zeros(1, 2, 1, 1), solver="dpm")
    server.run()
    assert float(a.result()[0, 0]) == 3 and float(b.result()[0, 0]) == 4
    assert float(b.result()[0, 1]) == float(sum(_dpm().schedule(4).timesteps))


# ------------------------------------------------------------------------------------------------ 3. the oracle itself
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("n", [5, 16])                 # 16 >= 15: lower_order_final no longer lowers the last steps
def test_oracle_sampler_follows_the_restated_solver(n, order):
    sched = _dpm(order).schedule(n)
    betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float32) ** 2
    ts = ref_timesteps(1000, n, "leading", 1)
    assert list(sched.timesteps) == [int(t) for t in ts]
    g = torch.Generator().manual_seed(10 * n + order)
    x = torch.randn(1, 4, 6, 6, generator=g, dtype=torch.float64)
    bias = torch.randn(1, 4, 6, 6, generator=g, dtype=torch.float64)

    def eps_fn(z, t):                                  # a made-up linear model: the solver's feedback loop is closed
        return 0.3 * z + (t / 1000.0) * bias

    ref = RefSolver(ref_sigmas(betas, ts, "zero"), order, "dpmsolver++", "midpoint", "epsilon")
    xr, outs_max = x, 0.0
    for t in ts:
        out = eps_fn(xr, int(t))
        outs_max = max(outs_max, float(out.abs().max()))
        xr = ref.step(out, xr)
    got = sdo.sample_with(eps_fn, x, sched)
    assert torch.isfinite(got).all(), "the NaN the history starts with must reach nothing"
    table = torch.tensor(sched.rows, dtype=torch.float64)
    # tests/test_dpm_host.py's bound for its row check, at the last step
    scale = (float(x.abs().max()) + outs_max) * max(1.0, float(table.abs().max()))
    err = float((got - xr).abs().max())
    print(f"[slots dpm host] n={n} order={order}: max |difference| {err:.2e}, bound {2e-6 * scale * n:.2e}")
    assert err <= 2e-6 * scale * n, (n, order, err, scale)


def test_oracle_step_leaves_the_other_slots_alone():
    g = torch.Generator().manual_seed(3)
    x, eps, hist = torch.randn(3, 2, 2, 2, generator=g), torch.randn(3, 2, 2, 2, generator=g), torch.randn(2, 3, 2, 2, 2, generator=g)
    hist[1, 1] = float("nan")                          # slot 1's h2: its row has b2 = 0
    coef = torch.tensor([[1.1, 0.2, 0.9, 0.3, 0, 0, 0, 0], [0.5, -0.4, 0.8, 0.7, 0.25, 0.0, 0, 0]])
    kind = torch.tensor([0, 1], dtype=torch.int32)
    pos, active = torch.tensor([0, 1, 1], dtype=torch.int32), torch.tensor([1, 1, 0], dtype=torch.int32)
    out, h = sdo.step_kinds(x, eps, hist, coef, kind, pos, active)
    assert torch.equal(out[2], x[2].double()) and torch.equal(h[:, 0], hist[:, 0].double())
    assert torch.equal(h[0, 2], hist[0, 2].double()) and torch.equal(h[1, 2], hist[1, 2].double())
    m0 = 0.5 * x[1].double() + float(coef[1, 1]) * eps[1].double()
    assert torch.allclose(h[0, 1], m0) and torch.equal(h[1, 1], hist[0, 1].double())
    assert torch.allclose(out[1], float(coef[1, 2]) * x[1].double() + float(coef[1, 3]) * m0 + 0.25 * hist[0, 1].double())
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ 4. the binding
def test_the_kinds_entry_point_is_declared_built_bound_and_documented():
    """afldm_slot_step_kinds lives in a library of its own: include/afldm_hip_slots.h <-> libafldm_slots.so, same symbols; the
    product header and library do not carry it, and importing the package does not load it."""
    import os
    import re
    import subprocess
    import sys
    from afldm_amd import _lib, _slots, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "afldm_hip_slots.h")).read()
    declared = set(re.findall(r"^int\s+(afldm_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert declared == {"afldm_slot_step_kinds"} == set(_slots.exports()) == set(_lib.SLOTS_ABI.functions)
    nm = subprocess.run(["nm", "-D", "--defined-only", _slots.SLOTS_PATH], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if " T afldm_" in l} == declared
    m = re.search(r"^int afldm_slot_step_kinds\(([^;]*)\);", hdr, re.M)
    params = [p.split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["x", "eps", "hist", "row_coef", "row_kind", "pos", "active", "B", "R", "C", "H", "W", "dtype", "stream"]
    assert len(_slots.lib().afldm_slot_step_kinds.argtypes) == len(params)
    assert "afldm_slot_step_kinds" not in _lib.EXPORTS and "slot_kinds.hip" in build.SLOTS_SOURCES and callable(ops.slot_step_kinds)
    assert "afldm_slot_step_kinds" in open(os.path.join(root, "INTEGRATION.md")).read()
    # refusals before any launch
    assert _slots.lib().afldm_slot_step_kinds(None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 0, None) == -5
    assert _slots.lib().afldm_slot_step_kinds(16, 16, 16, 16, 16, 16, 16, 0, 1, 1, 1, 1, 0, None) == -1
    assert b"afldm_slot_step_kinds" in _lib.lib.afldm_last_error()
    code = ("import sys; sys.path.insert(0, %r); import afldm_amd, afldm_amd.ops, afldm_amd.engine, afldm_amd.serving; "
            "print(any('libafldm_slots' in l for l in open('/proc/self/maps')))" % root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert r.stdout.strip().splitlines()[-1] == "False", r.stdout
