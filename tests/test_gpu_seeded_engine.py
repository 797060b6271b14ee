"""Seeded stochastic sampling end to end on MI355X: SeededEngine, MyLDMPipeline.sample_seeded and a SamplingServer with
kinds=("ddim", "dpm", "seeded") on the tiny UNet, against the CPU sampler of tests/noise_oracle.py (one request at a time on the
oracle UNet, its own seed), the eager launches and each other.  Bounds against the CPU samplers: the project's sampler bounds
(as tests/test_gpu_slot_engine_dpm.py) - rel-RMS <= 1e-3 for the fp32 model, <= 5e-2 for the bf16 model.  Everything else is bit
for bit: a request's noise is a function of its seed, the step and the element alone."""
import pytest
import torch

import noise_oracle as no
import slot_dpm_oracle as sdo
import slot_oracle as so
from test_gpu_sde import _ldm
from test_gpu_unet import build, rel_rms

pytestmark = pytest.mark.gpu

SHAPE = (1, 4, 16, 16)
SEEDS = [11, (1 << 40) + 5, 12345, 0]
KINDS = ("ddim", "dpm", "seeded")


def _ddim():
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    return ffhq_ddim_scheduler()


def _dpm():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, solver_order=2)


def _start(seed):
    from afldm_amd.utils import randn_tensor
    return randn_tensor(SHAPE, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def tiny32():
    return build("tiny", torch.float32)


@pytest.fixture(scope="module")
def ref(tiny32):
    """ref(kind, n, seed, eta): the CPU sampler's latents of an n-step request that starts from _start(seed); each computed once,
    shared, never written."""
    _, cfg, sd = tiny32
    made = {}

    def get(kind, n, seed, eta=0.0):
        key = (kind, n, seed, eta)
        if key not in made:
            if kind == "seeded":
                made[key] = no.sample(sd, cfg, _start(seed), _ddim().seeded_schedule(n, eta), seed)
            elif kind == "dpm":
                made[key] = sdo.sample(sd, cfg, _start(seed), _dpm().schedule(n))
            else:
                made[key] = so.sample(sd, cfg, _start(seed), _ddim().schedule(n))
        return made[key]
    return get


def _engine(unet, use_graph=True, steps_per_graph=2, n=6, eta=0.7, batch=4):
    from afldm_amd.engine import SeededEngine
    return SeededEngine(unet, _ddim().seeded_schedule(n, eta), batch, n, use_graph, steps_per_graph)


@pytest.fixture(scope="module")
def engine_run(tiny32):
    """SeededEngine at batch 4, 6 steps, eta = 0.7, 2 steps per graph: (start latents, the result on the host)."""
    x = torch.cat([_start(s) for s in SEEDS])
    eng = _engine(tiny32[0])
    out = eng.run(x, known=SEEDS)
    assert eng.noise is None and eng.graph is not None and eng.seeds.cpu().tolist() == SEEDS
    return x, out.cpu(), eng


# ------------------------------------------------------------------------------------------------ 1. the engine
def test_engine_against_the_cpu_sampler(engine_run, ref):
    _, out, _ = engine_run
    errs = [rel_rms(out[i:i + 1], ref("seeded", 6, s, 0.7)) for i, s in enumerate(SEEDS)]
    print("[seeded engine] fp32, batch 4, 6 steps, eta 0.7: rel-RMS against the CPU sampler " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-3, errs
    # the noise matters: the deterministic sampler from the same start is somewhere else
    assert rel_rms(out[:1], ref("ddim", 6, SEEDS[0])) > 1e-2


def test_graph_eager_grouping_and_repeat_are_bit_identical(tiny32, engine_run):
    x, out, eng = engine_run
    assert torch.equal(eng.run(x, known=torch.tensor(SEEDS)).cpu(), out), "a second run with the same seeds"
    assert torch.equal(_engine(tiny32[0], use_graph=False).run(x, known=SEEDS).cpu(), out), "graph replay against eager launches"
    assert torch.equal(_engine(tiny32[0], steps_per_graph=1).run(x, known=SEEDS).cpu(), out), "1 against 2 steps per graph"


def test_permuting_seeds_and_latents_permutes_the_output(engine_run):
    x, out, eng = engine_run
    perm = [2, 0, 3, 1]
    got = eng.run(x[perm], known=[SEEDS[i] for i in perm]).cpu()
    assert torch.equal(got, out[perm])
    # other seeds on the same start latents: other samples, from the same graphs
    graph = eng.graph
    other = eng.run(x, known=[s + 1 for s in SEEDS]).cpu()
    assert eng.graph is graph and not torch.equal(other, out)


def test_engine_refusals(tiny32, engine_run):
    from afldm_amd.engine import DenoiseEngine, SeededEngine
    x, _, eng = engine_run
    with pytest.raises(ValueError, match="seed"):
        eng.run(x)
    for bad in ([1, 2, 3], [1, 2, 3, -4], [1, 2, 3, 2 ** 63], [1, 2, 3, 0.5]):
        with pytest.raises(ValueError, match="seeds"):
            eng.run(x, known=bad)
    with pytest.raises(NotImplementedError, match="update_kind"):
        SeededEngine(tiny32[0], _ddim().stochastic_schedule(3, 0.5), 2, 3)
    with pytest.raises(NotImplementedError, match="update_kind"):
        DenoiseEngine(tiny32[0], _ddim().seeded_schedule(3, 0.5), 2, 3)
    assert "seeded" not in DenoiseEngine.UPDATES


def test_engine_after_a_dtype_change(ref):
    unet, _, _ = build("tiny", torch.float32)
    eng = _engine(unet)
    x = torch.cat([_start(s) for s in SEEDS])
    eng.run(x, known=SEEDS)
    unet.to(torch.bfloat16)
    out = eng.run(x, known=SEEDS).cpu()
    assert eng.x_nhwc.dtype == torch.bfloat16 and eng.seeds.cpu().tolist() == SEEDS
    errs = [rel_rms(out[i:i + 1], ref("seeded", 6, s, 0.7)) for i, s in enumerate(SEEDS)]
    print("[seeded engine] bf16 after unet.to(torch.bfloat16): rel-RMS against the CPU sampler " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 5e-2, errs


# ------------------------------------------------------------------------------------------------ 2. the pipeline
def test_sample_seeded(tiny32, engine_run):
    pipe = _ldm(tiny32[0])
    _, out, _ = engine_run
    got = pipe.sample_seeded(SEEDS, eta=0.7, num_inference_steps=6, output_type="latent")
    assert got.is_cuda and torch.equal(got.cpu(), out), "the pipeline draws sample i's start from manual_seed(seeds[i])"
    eager = pipe.sample_seeded(SEEDS, eta=0.7, num_inference_steps=6, use_graph=False, output_type="latent")
    err = rel_rms(eager, out)
    print(f"[seeded engine] sample_seeded(use_graph=False) against the graph path: rel-RMS {err:.2e}")
    assert err <= 1e-3
    # eta = 0: the plain sampler from the same start latents, exactly
    plain = pipe(batch_size=4, num_inference_steps=6, generator=[torch.Generator().manual_seed(s) for s in SEEDS], output_type="latent")
    assert torch.equal(pipe.sample_seeded(SEEDS, eta=0.0, num_inference_steps=6, output_type="latent"), plain)
    pipe.scheduler = _dpm()
    with pytest.raises(NotImplementedError, match="DDIMScheduler"):
        pipe.sample_seeded(SEEDS, num_inference_steps=6, output_type="latent")


# ------------------------------------------------------------------------------------------------ 3. the server
def _serve(unet, requests, slots, steps_per_graph=2, **kw):
    """requests: (steps, solver, eta, seed) in arrival order; each starts from _start(seed)."""
    from afldm_amd.serving import SamplingServer
    server = SamplingServer(_ldm(unet), slots, steps_per_graph, kinds=KINDS, **kw)
    tickets = [server.submit(n, solver=solver, eta=eta, seed=seed) for n, solver, eta, seed in requests]
    server.run()
    return server, tickets


def test_all_three_kinds_in_one_batch(tiny32, ref):
    requests = [(4, "ddim", 0.0, 21), (3, None, 0.5, 22), (5, "dpm", 0.0, 23), (6, None, 1.0, 24), (2, None, 0.5, 25)]
    server, tickets = _serve(tiny32[0], requests, 2)
    eng = server.engines[0]
    assert type(eng).__name__ == "SeededSlotEngine" and eng.table.kinds == KINDS and eng.hist is not None
    assert [eng.table.kind[t._span[0]] for t in tickets] == [0, 2, 1, 2, 2] and server.useful == sum(r[0] for r in requests)
    assert eng.row_ord.cpu().tolist()[:len(eng.table.ord)] == eng.table.ord
    errs = []
    for ticket, (n, solver, eta, seed) in zip(tickets, requests):
        got = ticket.result()
        assert got.dtype == torch.float32 and tuple(got.shape) == SHAPE and not got.is_cuda
        errs.append(rel_rms(got, ref("seeded" if eta else solver, n, seed, eta)))
    print("[seeded engine] DDIM 4, seeded 3, DPM 5, seeded 6, seeded 2 on 2 slots: rel-RMS against the CPU samplers "
          + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-3, errs


def test_seeded_slots_in_phase_against_the_engine(tiny32, engine_run):
    _, out, _ = engine_run
    _, tickets = _serve(tiny32[0], [(6, None, 0.7, s) for s in SEEDS], 4)
    got = torch.cat([t.result() for t in tickets])
    print(f"[seeded engine] four seeded slots in phase against SeededEngine at batch 4: max |difference| {float((got - out).abs().max()):.2e}")
    assert torch.equal(got, out)


def test_a_request_does_not_depend_on_its_slot_or_its_neighbours(tiny32):
    _, (alone,) = _serve(tiny32[0], [(5, None, 0.8, 77)], 2)
    others = [(3, "ddim", 0.0, 31), (4, None, 1.0, 32), (2, "dpm", 0.0, 33), (6, None, 0.3, 34)]
    server, tickets = _serve(tiny32[0], others + [(5, None, 0.8, 77)], 2)
    diff = float((tickets[-1].result() - alone.result()).abs().max())
    print(f"[seeded engine] one seeded request alone and last among four others on 2 slots: max |difference| {diff:.2e}")
    assert torch.equal(tickets[-1].result(), alone.result())


def test_slot_engine_refusals(tiny32):
    from afldm_amd.engine import SeededSlotEngine, SlotEngine
    eng = SeededSlotEngine(tiny32[0], 2, row_capacity=16, temb_capacity=16)
    assert eng.table.kinds == ("ddim", "seeded") and SlotEngine.TABLE.KIND_CODES == {"ddim": 0, "dpm": 1}
    with pytest.raises(NotImplementedError, match="schedules only"):
        eng.add_schedule(_ddim().stochastic_schedule(3, 0.5))
    with pytest.raises(NotImplementedError, match="schedules only"):
        eng.add_schedule(_dpm().schedule(3))
    span = eng.add_schedule(_ddim().seeded_schedule(3, 0.5))
    assert span == (0, 3) and eng.row_kind.cpu().tolist()[:3] == [2, 2, 2] and eng.row_ord.cpu().tolist()[:3] == [0, 1, 2]
    with pytest.raises(ValueError, match="seed"):
        eng.exchange({}, {0: (_start(1)[0], *span)})
    with pytest.raises(ValueError, match="seed"):
        eng.exchange({}, {0: (_start(1)[0], *span, -1)})
    assert not eng._busy and eng.seeds.cpu().tolist() == [0, 0]
    with pytest.raises(ValueError, match="kinds"):
        SlotEngine(tiny32[0], 2, kinds=("ddim", "seeded"))
