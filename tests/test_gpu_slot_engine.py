"""The slot sampler end to end on MI355X: SlotEngine and SamplingServer on the tiny UNet with the FFHQ DDIM scheduler against the
CPU sampler of tests/slot_oracle.py (one request at a time on the oracle UNet), the eager launches, the plain DenoiseEngine
and the pipeline's own calls.  Bounds: the project's sampler bounds - rel-RMS <= 1e-3 for the fp32 model, <= 5e-2
for the bf16 model.

Measured on MI355X (rel-RMS; against the CPU sampler unless said otherwise):
  test 1, fp32, six requests of (3, 5, 2, 4, 3, 5) steps on 4 slots:  8.1e-8 ... 1.08e-7; graph, eager, 1 step per graph: the same bits
  test 4, inversion next to sampling, against pipe.ddim_inversion:     0 (bit-identical)
  test 5, four slots in phase against DenoiseEngine at batch 4:         0, max |difference| 0
  test 6, eight requests on 2 x 2 slots: 7.9e-8 ... 1.08e-7;  sample_mixed against three pipe(batch_size=1) calls: 0
  test 7, the bf16 model after unet.to(torch.bfloat16):                3.4e-4 ... 4.4e-4"""
import pytest
import torch

import slot_oracle as so
from test_gpu_sde import _ldm
from test_gpu_unet import build, rel_rms

pytestmark = pytest.mark.gpu

STEPS = (3, 5, 2, 4, 3, 5, 2, 4)            # test 1 takes the first six
SHAPE = (1, 4, 16, 16)


def _start(i):
    from afldm_amd.utils import randn_tensor
    return randn_tensor(SHAPE, generator=torch.Generator().manual_seed(100 + i))


@pytest.fixture(scope="module")
def tiny32():
    return build("tiny", torch.float32)


@pytest.fixture(scope="module")
def refs(tiny32):
    """The CPU sampler's latents of the eight requests: computed once, shared, never written."""
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    _, cfg, sd = tiny32
    return [so.sample(sd, cfg, _start(i), ffhq_ddim_scheduler().schedule(n)) for i, n in enumerate(STEPS)]


def _serve(unet, steps, slots, steps_per_graph, engines=1, use_graph=True):
    from afldm_amd.serving import SamplingServer
    server = SamplingServer(_ldm(unet), slots, steps_per_graph, engines, use_graph=use_graph)
    tickets = [server.submit(n, generator=torch.Generator().manual_seed(100 + i)) for i, n in enumerate(steps)]
    server.run()
    return server, tickets


def _check(tickets, refs, tol, what):
    errs = []
    for ticket, ref in zip(tickets, refs):
        got = ticket.result()
        assert ticket.done() and got.dtype == torch.float32 and tuple(got.shape) == SHAPE and not got.is_cuda
        errs.append(rel_rms(got, ref))
    print(f"[slot engine] {what}: rel-RMS against the CPU sampler " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= tol, errs
    return errs


# ------------------------------------------------------------------------------------------------ 1. and 2.
def test_mixed_requests_against_the_cpu_sampler_and_graph_against_eager(tiny32, refs):
    server, tickets = _serve(tiny32[0], STEPS[:6], 4, 2)
    eng = server.engines[0]
    assert eng.graph is not None and eng.graph_multi is not None and eng.branches == 1
    assert server.useful == sum(STEPS[:6]) and server.evaluations > server.useful          # some requests finish mid-group
    assert len(eng.table.spans) == 4 and len(eng.table.t) == 2 + 3 + 4 + 5                     # four step counts, each stored once
    _check(tickets, refs, 1e-3, "fp32, (3, 5, 2, 4, 3, 5) steps on 4 slots, 2 steps per graph")
    _, eager = _serve(tiny32[0], STEPS[:6], 4, 2, use_graph=False)
    for a, b in zip(tickets, eager):
        assert torch.equal(a.result(), b.result()), "graph replay must be bit-identical to eager launches"
    # any grouping gives the same latents
    _, single = _serve(tiny32[0], STEPS[:6], 4, 1)
    for a, b in zip(tickets, single):
        assert torch.equal(a.result(), b.result())


# ------------------------------------------------------------------------------------------------ 3. a finished slot is frozen
def test_frozen_slot(tiny32, refs):
    from afldm_amd.serving import SamplingServer
    server = SamplingServer(_ldm(tiny32[0]), 2, 3)
    short = server.submit(2, generator=torch.Generator().manual_seed(102))          # request 2 of STEPS: 2 steps
    long_ = server.submit(6, generator=torch.Generator().manual_seed(7))
    eng = server.engines[0]
    assert server.poll(max_replays=1) == 1                # one 3-step group: the short request ends after 2 of them
    first = eng.lat[0].clone()
    pos = eng.pos.cpu().tolist()
    assert server.poll(max_replays=1) == 1
    second = eng.lat[0].clone()
    assert torch.equal(first, second) and eng.pos.cpu().tolist() == [pos[0], pos[1] + 3]
    server.run()
    assert torch.equal(short.result()[0], first.cpu()) and rel_rms(short.result(), refs[2]) <= 1e-3
    assert torch.isfinite(long_.result()).all() and server.useful == 8 and server.evaluations == 12


# ------------------------------------------------------------------------------------------------ 4. inversion next to sampling
def test_inversion_and_sampling_in_one_batch(tiny32, refs):
    from afldm_amd.serving import SamplingServer
    pipe = _ldm(tiny32[0])
    pipe.scheduler.set_timesteps(4)
    inv = pipe.inversion_schedule()
    x = _start(50)
    want = pipe.ddim_inversion(x.cuda(), bar=False)
    server = SamplingServer(pipe, 3, 2)
    a = server.submit(STEPS[0], generator=torch.Generator().manual_seed(100))
    t = server.submit(schedule=inv, latents=x)
    b = server.submit(STEPS[1], generator=torch.Generator().manual_seed(101))
    server.run()
    err = rel_rms(t.result(), want.cpu())
    print(f"[slot engine] 4-step inversion between two sampling requests: rel-RMS against pipe.ddim_inversion {err:.2e}")
    assert err <= 1e-3, err
    _check([a, b], refs[:2], 1e-3, "the sampling requests next to it")


# ------------------------------------------------------------------------------------------------ 5. in phase: the plain engine
def test_slots_in_phase_against_the_plain_engine(tiny32):
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.serving import SamplingServer
    x = torch.cat([_start(i) for i in range(4)])
    want = DenoiseEngine(tiny32[0], ffhq_ddim_scheduler(), 4, 5).run(x)
    server = SamplingServer(_ldm(tiny32[0]), 4, 5)
    tickets = [server.submit(5, latents=x[i:i + 1]) for i in range(4)]
    server.run()
    got = torch.cat([t.result() for t in tickets])
    err, worst = rel_rms(got, want.cpu()), float((got - want.cpu()).abs().max())
    print(f"[slot engine] four slots in phase, 5 steps, against DenoiseEngine at batch 4: rel-RMS {err:.2e}, max |difference| {worst:.2e}")
    assert err <= 1e-3, err
    assert server.evaluations == server.useful == 20 and server.replays == 1


# ------------------------------------------------------------------------------------------------ 6. two engines; the pipeline
def test_two_engines_and_the_pipeline_method(tiny32, refs):
    server, tickets = _serve(tiny32[0], STEPS, 2, 2, engines=2)
    assert len(server.engines) == 2 and [t.engine for t in tickets] == [0, 1] * 4
    _check(tickets, refs, 1e-3, "fp32, eight requests on 2 x 2 slots")
    pipe = _ldm(tiny32[0])
    counts = [2, 4, 3]
    got = pipe.sample_mixed(counts, generator=[torch.Generator().manual_seed(40 + i) for i in range(3)], output_type="latent")
    assert tuple(got.shape) == (3, 4, 16, 16) and got.is_cuda
    errs = []
    for i, n in enumerate(counts):
        one = pipe(batch_size=1, num_inference_steps=n, generator=torch.Generator().manual_seed(40 + i), output_type="latent")
        errs.append(rel_rms(got[i:i + 1], one.cpu()))
    print("[slot engine] sample_mixed([2, 4, 3]) against three pipe(batch_size=1) calls: rel-RMS " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-3, errs
    (server,) = pipe._slot_servers.values()
    again = pipe.sample_mixed(counts, generator=[torch.Generator().manual_seed(40 + i) for i in range(3)], output_type="latent")
    assert torch.equal(again, got) and next(iter(pipe._slot_servers.values())) is server


# ------------------------------------------------------------------------------------------------ 7. a dtype change
def test_after_a_dtype_change(refs):
    from afldm_amd.serving import SamplingServer
    unet, _, _ = build("tiny", torch.float32)
    server = SamplingServer(_ldm(unet), 4, 2)

    def round_():
        tickets = [server.submit(n, generator=torch.Generator().manual_seed(100 + i)) for i, n in enumerate(STEPS[:6])]
        server.run()
        return tickets
    _check(round_(), refs, 1e-3, "fp32, before the dtype change")
    eng = server.engines[0]
    graph = eng.graph
    unet.to(torch.bfloat16)
    tickets = round_()
    assert server.engines[0] is eng and eng.x_nhwc.dtype == eng.temb_rows.dtype == torch.bfloat16
    assert eng.graph is not None and eng.graph is not graph
    _check(tickets, refs, 5e-2, "bf16, after unet.to(torch.bfloat16)")


# ------------------------------------------------------------------------------------------------ what the engine refuses
def test_refusals(tiny32):
    from afldm_amd.engine import SlotEngine
    from afldm_amd.pipelines.cross_frame_attn import (AttnState, CrossFrameAttnProcessor, get_unet_attn_processors,
                                                      set_unet_attn_processor)
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    eng = SlotEngine(tiny32[0], 2, row_capacity=6, temb_capacity=8)
    with pytest.raises(NotImplementedError, match="'ddim' schedules only"):
        eng.add_schedule(ffhq_ddim_scheduler().stochastic_schedule(3, 0.5))
    assert eng.add_schedule(ffhq_ddim_scheduler().schedule(4)) == (0, 4)
    with pytest.raises(RuntimeError, match="row table is full"):
        eng.add_schedule(ffhq_ddim_scheduler().schedule(3))
    with pytest.raises(NotImplementedError):
        eng.run(torch.zeros(2, 4, 16, 16))
    unet, _, _ = build("tiny", torch.float32)
    state = AttnState()
    set_unet_attn_processor(unet, {k: CrossFrameAttnProcessor(state) for k in get_unet_attn_processors(unet)})
    with pytest.raises(ValueError, match="plain one"):
        SlotEngine(unet, 2)
