"""DPM-Solver++ requests in slots, end to end on MI355X: SlotEngine / SamplingServer with kinds=("ddim", "dpm") on the tiny UNet with
DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, solver_order=...) against the CPU sampler of tests/slot_dpm_oracle.py
(one request at a time on the oracle UNet, its own history), the eager launches, the plain DenoiseEngine and the pipeline's own
calls.  Bounds: the project's sampler bounds - rel-RMS <= 1e-3 for the fp32 model, <= 5e-2 for the bf16 model.

Measured on MI355X (rel-RMS against the CPU sampler; profiles/slots/test_gpu_slots_dpm.log):
  test 1, fp32, six requests of (3, 5, 2, 4, 16, 5) steps on 4 slots: order 2  7.3e-8 ... 1.8e-7, order 3  7.3e-8 ... 2.2e-7;
          graph, eager, 1 step per graph: the same bits
  test 2, four slots in phase against DenoiseEngine at batch 4: bit-identical
  test 3, DDIM 4, DPM 3, DDIM 2, DPM 5, DPM 2 on 2 slots: 7.5e-8 ... 1.2e-7
  test 4, the bf16 model after unet.to(torch.bfloat16): 2.4e-4 ... 3.8e-4
  test 5, sample_mixed([2, 4, 3]) against three pipe(batch_size=1) calls, DPM and then DDIM on the same pipe: 0"""
import pytest
import torch

import slot_dpm_oracle as sdo
import slot_oracle as so
from test_gpu_sde import _ldm
from test_gpu_unet import build, rel_rms

pytestmark = pytest.mark.gpu

STEPS = (3, 5, 2, 4, 16, 5)                # 16 >= 15: lower_order_final no longer lowers the last rows
SHAPE = (1, 4, 16, 16)
KINDS = ("ddim", "dpm")


def _start(i):
    from afldm_amd.utils import randn_tensor
    return randn_tensor(SHAPE, generator=torch.Generator().manual_seed(100 + i))


def _dpm(order):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, solver_order=order)


def _dpm_pipe(unet, order):
    pipe = _ldm(unet)
    pipe.scheduler = _dpm(order)
    return pipe


@pytest.fixture(scope="module")
def tiny32():
    return build("tiny", torch.float32)


@pytest.fixture(scope="module")
def ref(tiny32):
    """ref(solver, n, i, order=2): the CPU sampler's latents of an n-step request that starts from _start(i); each computed
    once, shared, never written."""
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    _, cfg, sd = tiny32
    made = {}

    def get(solver, n, i, order=2):
        key = (solver, n, i, order if solver == "dpm" else None)
        if key not in made:
            if solver == "dpm":
                made[key] = sdo.sample(sd, cfg, _start(i), _dpm(order).schedule(n))
            else:
                made[key] = so.sample(sd, cfg, _start(i), ffhq_ddim_scheduler().schedule(n))
        return made[key]
    return get


def _serve(pipe, requests, slots, steps_per_graph, use_graph=True, **kw):
    """requests: (steps, solver) in arrival order; request i starts from _start(i)."""
    from afldm_amd.serving import SamplingServer
    server = SamplingServer(pipe, slots, steps_per_graph, use_graph=use_graph, **kw)
    tickets = [server.submit(n, generator=torch.Generator().manual_seed(100 + i), solver=solver)
               for i, (n, solver) in enumerate(requests)]
    server.run()
    return server, tickets


def _check(tickets, refs, tol, what):
    errs = []
    for ticket, want in zip(tickets, refs):
        got = ticket.result()
        assert ticket.done() and got.dtype == torch.float32 and tuple(got.shape) == SHAPE and not got.is_cuda
        errs.append(rel_rms(got, want))
    print(f"[slot engine dpm] {what}: rel-RMS against the CPU sampler " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= tol, errs
    return errs


# ------------------------------------------------------------------------------------------------ 1. mixed DPM requests
@pytest.mark.parametrize("order", [2, 3])
def test_mixed_dpm_requests_against_the_cpu_sampler_and_graph_against_eager(tiny32, ref, order):
    requests = [(n, None) for n in STEPS]                                  # (the pipe's scheduler is a DPM one: its own class)
    server, tickets = _serve(_dpm_pipe(tiny32[0], order), requests, 4, 2)
    eng = server.engines[0]
    assert server.kinds == KINDS and eng.table.kinds == KINDS and eng.graph is not None and eng.graph_multi is not None
    assert tuple(eng.hist.shape) == (2, 4) + SHAPE[1:] and eng.hist.dtype == torch.float32 and tuple(eng.row_coef.shape[1:]) == (8,)
    assert any(t is eng.hist for t in eng._carried())
    assert server.useful == sum(STEPS) and server.evaluations > server.useful
    assert set(eng.table.kind) == {1} and len(eng.table.spans) == 5 and len(eng.table.t) == 2 + 3 + 4 + 5 + 16
    _check(tickets, [ref("dpm", n, i, order) for i, n in enumerate(STEPS)], 1e-3,
           f"fp32, order {order}, {STEPS} steps on 4 slots, 2 steps per graph")
    # the eager path has no warm-up step: a history that _capture did not put back would show here
    _, eager = _serve(_dpm_pipe(tiny32[0], order), requests, 4, 2, use_graph=False)
    for a, b in zip(tickets, eager):
        assert torch.equal(a.result(), b.result()), "graph replay must be bit-identical to eager launches"
    _, single = _serve(_dpm_pipe(tiny32[0], order), requests, 4, 1)
    for a, b in zip(tickets, single):
        assert torch.equal(a.result(), b.result()), "any grouping gives the same latents"


# ------------------------------------------------------------------------------------------------ 2. in phase: the plain engine
def test_dpm_slots_in_phase_against_the_plain_engine(tiny32):
    from afldm_amd.engine import DenoiseEngine
    x = torch.cat([_start(i) for i in range(4)])
    want = DenoiseEngine(tiny32[0], _dpm(3), 4, 5).run(x)
    _, tickets = _serve(_dpm_pipe(tiny32[0], 3), [(5, None)] * 4, 4, 5)
    got = torch.cat([t.result() for t in tickets])
    err, worst = rel_rms(got, want.cpu()), float((got - want.cpu()).abs().max())
    print(f"[slot engine dpm] four slots in phase, 5 steps of order 3, against DenoiseEngine at batch 4: rel-RMS {err:.2e}, "
          f"max |difference| {worst:.2e}")
    assert torch.equal(got, want.cpu()), (err, worst)


# ------------------------------------------------------------------------------------------------ 3. both solvers in one batch
def test_both_solvers_in_one_batch(tiny32, ref):
    # on 2 slots every slot holds a DPM request after a DDIM one and a DPM one after a DPM one; nothing clears a history
    requests = [(4, "ddim"), (3, "dpm"), (2, "ddim"), (5, "dpm"), (2, "dpm")]
    server, tickets = _serve(_ldm(tiny32[0]), requests, 2, 2, kinds=KINDS)
    eng = server.engines[0]
    assert set(eng.table.kind) == {0, 1} and server.useful == sum(n for n, _ in requests)
    order = [(eng.table.kind[t._span[0]], t._span) for t in tickets]
    assert [k for k, _ in order] == [0, 1, 0, 1, 1]
    _check(tickets, [ref(solver, n, i) for i, (n, solver) in enumerate(requests)], 1e-3,
           "fp32, DDIM 4, DPM 3, DDIM 2, DPM 5, DPM 2 on 2 slots")


# ------------------------------------------------------------------------------------------------ 4. a dtype change
def test_after_a_dtype_change(ref):
    from afldm_amd.serving import SamplingServer
    unet, _, _ = build("tiny", torch.float32)
    server = SamplingServer(_dpm_pipe(unet, 2), 4, 2)
    refs = [ref("dpm", n, i) for i, n in enumerate(STEPS)]

    def round_():
        tickets = [server.submit(n, generator=torch.Generator().manual_seed(100 + i)) for i, n in enumerate(STEPS)]
        server.run()
        return tickets
    _check(round_(), refs, 1e-3, "fp32, before the dtype change")
    eng = server.engines[0]
    graph, hist = eng.graph, eng.hist
    unet.to(torch.bfloat16)
    tickets = round_()
    assert server.engines[0] is eng and eng.x_nhwc.dtype == torch.bfloat16
    assert eng.hist is not hist and eng.hist.dtype == torch.float32 and tuple(eng.hist.shape) == tuple(hist.shape)
    assert eng.graph is not None and eng.graph is not graph and any(t is eng.hist for t in eng._carried())
    _check(tickets, refs, 5e-2, "bf16, after unet.to(torch.bfloat16)")


# ------------------------------------------------------------------------------------------------ 5. the pipeline
def test_pipeline_method_with_a_dpm_scheduler_and_back(tiny32):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = _dpm_pipe(tiny32[0], 2)
    counts = [2, 4, 3]

    def gens():
        return [torch.Generator().manual_seed(40 + i) for i in range(3)]

    def against_single_calls(got, what):
        errs = []
        for i, n in enumerate(counts):
            one = pipe(batch_size=1, num_inference_steps=n, generator=gens()[i], output_type="latent")
            errs.append(rel_rms(got[i:i + 1], one.cpu()))
        print(f"[slot engine dpm] sample_mixed({counts}), {what}, against three pipe(batch_size=1) calls: rel-RMS "
              + " ".join(f"{e:.2e}" for e in errs))
        assert max(errs) <= 1e-3, errs
    got = pipe.sample_mixed(counts, generator=gens(), output_type="latent")
    assert tuple(got.shape) == (3, 4, 16, 16) and got.is_cuda
    (dpm_server,) = pipe._slot_servers.values()
    assert dpm_server.kinds == KINDS and set(dpm_server.engines[0].table.kind) == {1}
    against_single_calls(got, "DPM scheduler")
    # the DDIM scheduler back on the same pipe: a server of its own, and the answers of tests/test_gpu_slot_engine.py's test 6
    pipe.scheduler = ffhq_ddim_scheduler()
    ddim = pipe.sample_mixed(counts, generator=gens(), output_type="latent")
    (ddim_server,) = pipe._slot_servers.values()
    assert ddim_server is not dpm_server and ddim_server.kinds == ("ddim",) and ddim_server.engines[0].hist is None
    assert not torch.equal(ddim, got)
    against_single_calls(ddim, "DDIM scheduler")
    again = pipe.sample_mixed(counts, generator=gens(), output_type="latent")
    assert torch.equal(again, ddim) and next(iter(pipe._slot_servers.values())) is ddim_server
    # and DPM again: the DDIM server cannot take these, so it must not be the one that is asked
    pipe.scheduler = _dpm(2)
    assert torch.equal(pipe.sample_mixed(counts, generator=gens(), output_type="latent"), got)


# ------------------------------------------------------------------------------------------------ the carried history
def test_a_capture_in_the_middle_of_a_schedule_keeps_the_history(tiny32):
    """_capture runs a warm-up step and puts the carried buffers back.  At a server's first capture every occupied slot stands
    before its first row, whose zero coefficients hide a history shifted once too often; a capture with slots in the middle of
    their schedules (the graphs are dropped when a hand-over error is reported, DenoiseEngine.check_errors) does not hide it."""
    from afldm_amd.engine import SlotEngine
    sched = _dpm(3).schedule(6)
    x = torch.cat([_start(i) for i in range(2)])

    def engine(use_graph):
        eng = SlotEngine(tiny32[0], 2, use_graph, 2, kinds=KINDS)
        span = eng.add_schedule(sched)
        eng.exchange({}, {b: (x[b], *span) for b in range(2)})
        return eng
    eager, graphs = engine(False), engine(True)
    eager.step(6)
    graphs.step(3)
    assert graphs.graph is not None
    graphs.graph = graphs.graph_multi = None               # as check_errors drops them: the next step captures again, at row 3
    graphs.step(3)
    assert graphs.graph is not None and graphs.pos.cpu().tolist() == eager.pos.cpu().tolist() == [5, 5]
    assert torch.equal(graphs.lat, eager.lat) and torch.equal(graphs.hist, eager.hist)


# ------------------------------------------------------------------------------------------------ 6. what is refused
def test_refusals(tiny32):
    from afldm_amd.engine import SlotEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.serving import SamplingServer
    eng = SlotEngine(tiny32[0], 2, row_capacity=8, temb_capacity=8, kinds=KINDS)
    with pytest.raises(NotImplementedError, match="'ddim' schedules only"):
        eng.add_schedule(ffhq_ddim_scheduler().stochastic_schedule(3, 0.5))
    assert eng.add_schedule(_dpm(2).schedule(4)) == (0, 4) and eng.add_schedule(ffhq_ddim_scheduler().schedule(3)) == (4, 7)
    assert eng.row_kind.cpu().tolist() == [1, 1, 1, 1, 0, 0, 0, 0] and (eng.row_coef[4:7, 4:] == 0).all()
    with pytest.raises(ValueError, match="kinds"):
        SlotEngine(tiny32[0], 2, kinds=("ddim", "sde"))
    server = SamplingServer(_ldm(tiny32[0]), 2, 2)
    assert server.kinds == ("ddim",) and server.engines[0].hist is None and tuple(server.engines[0].row_coef.shape[1:]) == (4,)
    with pytest.raises(NotImplementedError, match="'ddim' schedules only"):
        server.submit(3, solver="dpm")
    assert not server._queue[0]
