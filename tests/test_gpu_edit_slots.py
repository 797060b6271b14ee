"""Image-conditioned requests in slots end to end on MI355X: EditSlotEngine and a SamplingServer with the edit kinds on the tiny
UNet, against the CPU samplers of tests/edit_oracle.py (one request at a time on the oracle UNet, float64 latents, the noise of
noise_oracle.normals), the plain pipeline, and each other.  Bounds against the CPU samplers and the plain pipeline: the project's
sampler bounds (as tests/test_gpu_seeded_engine.py) - rel-RMS <= 1e-3 for the fp32 model, <= 5e-2 for the bf16 model.  Everything
else is bit for bit: a request's result is a function of the request alone.

Latents [1, 4, 16, 16]; img2img over n = 6 with strength 0.7 (4 evaluations); RePaint over n = 6 with jump_length = 2,
jump_n_sample = 2 (10 evaluations); 2 to 4 slots."""
import pytest
import torch

import edit_oracle as eo
import noise_oracle as no
import slot_dpm_oracle as sdo
import slot_oracle as so
from test_gpu_sde import _ldm
from test_gpu_seeded_engine import _ddim, _dpm, _start
from test_gpu_unet import build, rel_rms

pytestmark = pytest.mark.gpu

SHAPE = (1, 4, 16, 16)
KINDS = ("ddim", "dpm", "seeded", "seeded_sdedit", "seeded_repaint")
N, STRENGTH, JL, JS = 6, 0.7, 2, 2


def _planes(seed):
    """(latents, soft map, hard mask) of a request: the map has exact 0s, exact 1s and values between; the mask is 0 / 1."""
    g = torch.Generator().manual_seed(1000 + seed)
    lat = torch.randn(SHAPE, generator=g)
    soft = torch.rand(1, 1, 16, 16, generator=g)
    soft[..., :5] = 0.0
    soft[..., 12:] = 1.0
    hard = torch.zeros(1, 1, 16, 16)
    hard[..., 3:11, :9] = 1.0
    return lat, soft, hard


@pytest.fixture(scope="module")
def tiny32():
    return build("tiny", torch.float32)


def _submit(server, req):
    """req: ("img2img", seed, eta, map name) | ("inpaint", seed, eta, mask name) | ("txt", n, solver, eta, seed)."""
    if req[0] == "txt":
        _, n, solver, eta, seed = req
        return server.submit(n, solver=solver, eta=eta, seed=seed)
    what, seed, eta, which = req
    lat, soft, hard = _planes(seed)
    m = {"soft": soft, "hard": hard, "none": None, "zero": torch.zeros_like(soft)}[which]
    if what == "img2img":
        return server.submit_img2img_latents(lat, STRENGTH, m, N, eta, seed=seed)
    return server.submit_inpaint_latents(lat, m, N, eta, JL, JS, seed=seed)


def _serve(unet, requests, slots, steps_per_graph=2, **kw):
    from afldm_amd.serving import SamplingServer
    server = SamplingServer(_ldm(unet), slots, steps_per_graph, kinds=KINDS, **kw)
    tickets = [_submit(server, r) for r in requests]
    server.run()
    return server, tickets


def _cpu(sd, cfg, req):
    what, seed, eta, which = req
    lat, soft, hard = _planes(seed)
    m = {"soft": soft, "hard": hard, "none": torch.ones_like(soft)}[which]
    if what == "img2img":
        sched = _ddim().seeded_sdedit_schedule(N, STRENGTH, eta)
        start = eo.sdedit_start(lat, *_ddim().sdedit_start(N, STRENGTH), seed)
        return eo.sample_sdedit(sd, cfg, lat, m, sched, start, seed)
    return eo.sample_repaint(sd, cfg, _start(seed), lat, m, _ddim().seeded_repaint_schedule(N, eta, JL, JS), seed)


EDITS = [("img2img", 51, 0.5, "soft"), ("inpaint", 52, 0.5, "hard"), ("img2img", 53, 0.0, "none"), ("inpaint", 54, 0.0, "soft")]


@pytest.fixture(scope="module")
def cpu_refs(tiny32):
    """The CPU samplers' latents of EDITS, each computed once, shared, never written."""
    _, cfg, sd = tiny32
    return [_cpu(sd, cfg, r) for r in EDITS]


@pytest.fixture(scope="module")
def served(tiny32):
    """EDITS on a server of 2 slots, 2 steps per graph: (server, tickets)."""
    return _serve(tiny32[0], EDITS, 2)


# ------------------------------------------------------------------------------------------------ 1. against the CPU samplers
def test_edit_requests_against_the_cpu_samplers(served, cpu_refs):
    server, tickets = served
    eng = server.engines[0]
    assert type(eng).__name__ == "EditSlotEngine" and eng.table.kinds == KINDS and tuple(eng.row_coef.shape[1:]) == (12,)
    assert [t.steps for t in tickets] == [4, 10, 4, 10] and server.useful == 28
    assert [eng.table.kind[t._span[0]] for t in tickets] == [3, 4, 3, 4]
    errs = []
    for ticket, ref in zip(tickets, cpu_refs):
        got = ticket.result()
        assert got.dtype == torch.float32 and tuple(got.shape) == SHAPE and not got.is_cuda
        errs.append(rel_rms(got, ref))
    print("[edit slots] fp32, img2img eta 0.5 / inpaint eta 0.5 / img2img eta 0 / inpaint eta 0 on 2 slots: rel-RMS against the CPU "
          "samplers " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-3, errs
    # (another request's CPU sample is somewhere else)
    assert rel_rms(tickets[0].result(), cpu_refs[2]) > 1e-2


def test_edit_requests_in_bf16_against_the_cpu_samplers(cpu_refs):
    unet, _, _ = build("tiny", torch.bfloat16)
    _, tickets = _serve(unet, EDITS, 3)
    errs = [rel_rms(t.result(), ref) for t, ref in zip(tickets, cpu_refs)]
    print("[edit slots] bf16, the same four requests on 3 slots: rel-RMS against the CPU samplers " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 5e-2, errs


# ------------------------------------------------------------------------------------------------ 2. against the plain pipeline
def test_img2img_at_eta_0_against_the_plain_pipeline(tiny32, served):
    from afldm_amd import ops
    _, tickets = served
    _, seed, _, _ = EDITS[2]
    lat, _, _ = _planes(seed)
    z = ops.counter_noise(torch.tensor([seed], device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), SHAPE, slot=1)
    assert float((z.cpu().double() - torch.from_numpy(no.normals(seed, 0, z.numel(), 1)).reshape(SHAPE)).abs().max()) <= 1e-5
    plain = _ldm(tiny32[0]).img2img_latents(lat, STRENGTH, None, N, eta=0.0, noise=z)
    err = rel_rms(tickets[2].result(), plain.float().cpu())
    print(f"[edit slots] img2img at eta 0 in a slot against pipe.img2img_latents fed the materialised z: rel-RMS {err:.2e}")
    assert err <= 1e-3


# ------------------------------------------------------------------------------------------------ 3. invariances, bit for bit
OTHERS = [("txt", 3, "ddim", 0.0, 31), ("img2img", 57, 0.3, "soft"), ("txt", 4, None, 1.0, 32), ("txt", 2, "dpm", 0.0, 33),
          ("inpaint", 58, 0.7, "soft")]


@pytest.mark.parametrize("req", EDITS[:2], ids=["img2img", "inpaint"])
def test_an_edit_request_does_not_depend_on_slot_neighbours_grouping_or_replay(tiny32, served, req):
    _, tickets = served
    base = tickets[EDITS.index(req)].result()
    _, (alone,) = _serve(tiny32[0], [req], 2)
    assert torch.equal(alone.result(), base), "served alone against served among the four edit requests"
    server, among = _serve(tiny32[0], OTHERS + [req], 2)
    diff = float((among[-1].result() - base).abs().max())
    print(f"[edit slots] {req[0]} alone and last among five others of four kinds on 2 slots: max |difference| {diff:.2e}")
    assert torch.equal(among[-1].result(), base)
    assert sorted({server.engines[0].table.kind[t._span[0]] for t in among}) == [0, 1, 2, 3, 4]
    _, (regrouped,) = _serve(tiny32[0], [req], 2, steps_per_graph=3)
    assert torch.equal(regrouped.result(), base), "3 against 2 steps per graph"
    _, (eager,) = _serve(tiny32[0], [req], 2, use_graph=False)
    assert torch.equal(eager.result(), base), "graph replay against eager launches"


def test_the_other_kinds_keep_their_results_next_to_edit_requests(tiny32):
    """The txt / seeded / dpm requests of OTHERS, served among edit requests by an EditSlotEngine, against the CPU samplers."""
    _, cfg, sd = tiny32
    _, tickets = _serve(tiny32[0], OTHERS, 2)
    errs = []
    for ticket, req in zip(tickets, OTHERS):
        if req[0] != "txt":
            continue
        _, n, solver, eta, seed = req
        if eta:
            ref = no.sample(sd, cfg, _start(seed), _ddim().seeded_schedule(n, eta), seed)
        elif solver == "dpm":
            ref = sdo.sample(sd, cfg, _start(seed), _dpm().schedule(n))
        else:
            ref = so.sample(sd, cfg, _start(seed), _ddim().schedule(n))
        errs.append(rel_rms(ticket.result(), ref))
    print("[edit slots] DDIM 3, seeded 4, DPM 2 next to edit requests: rel-RMS against the CPU samplers " + " ".join(f"{e:.2e}" for e in errs))
    assert len(errs) == 3 and max(errs) <= 1e-3, errs


def test_two_engines_on_two_streams_give_the_same_results(tiny32, served):
    """engines=2: the requests are dealt out alternately to two engines on streams of their own; the planes and the img2img start are
    device tensors made on the caller's stream."""
    _, tickets = served
    _, dealt = _serve(tiny32[0], EDITS, 2, engines=2)
    assert [t.engine for t in dealt] == [0, 1, 0, 1]
    for got, want in zip(dealt, tickets):
        assert torch.equal(got.result(), want.result())


def test_submitting_between_polls_on_two_engines_gives_the_same_results(tiny32, served):
    """The way a server is driven: requests arrive between poll(max_replays=1) calls.  A request's device tensors - its start, its
    planes - are made on the caller's stream and read on its engine's at a later boundary, after the server has dropped them; the
    memory they leave must not be handed to a later request before that read (many requests of the same sizes, so that the
    allocator would reuse the blocks)."""
    from afldm_amd.serving import SamplingServer
    _, tickets = served
    server = SamplingServer(_ldm(tiny32[0]), 2, 2, engines=2, kinds=KINDS)        # (2 slots each, as `served`: the same batch)
    order = [0, 1, 2, 3, 1, 0, 3, 2, 0, 1, 2, 3]
    dealt = []
    for i in order:
        dealt.append(_submit(server, EDITS[i]))
        server.poll(max_replays=1)
    server.run()
    assert {t.engine for t in dealt} == {0, 1}
    for i, got in zip(order, dealt):
        assert torch.equal(got.result(), tickets[i].result()), i


# ------------------------------------------------------------------------------------------------ 4. exactness
def test_change_value_0_and_a_hard_mask_return_the_conditioning_exactly(tiny32, served):
    server, tickets = served
    lat, soft, _ = _planes(EDITS[0][1])
    keep = (soft == 0).expand(SHAPE)
    got = tickets[0].result()
    assert torch.equal(got[keep], lat[keep]) and not torch.equal(got[~keep], lat[~keep]) and keep.any()
    lat, _, hard = _planes(EDITS[1][1])
    keep = (hard == 1).expand(SHAPE)
    got = tickets[1].result()
    assert torch.equal(got[keep], lat[keep]) and not torch.equal(got[~keep], lat[~keep]) and keep.any()
    # a map of zeros everywhere: the original, whatever the UNet says
    _, (same,) = _serve(tiny32[0], [("img2img", 51, 0.5, "zero")], 2)
    assert torch.equal(same.result(), _planes(51)[0])


def test_other_seeds_give_other_samples_from_the_same_graphs(tiny32):
    from afldm_amd.serving import SamplingServer
    server = SamplingServer(_ldm(tiny32[0]), 2, 2, kinds=KINDS)
    lat, soft, hard = _planes(61)
    first = [server.submit_img2img_latents(lat, STRENGTH, soft, N, 0.5, seed=1), server.submit_inpaint_latents(lat, hard, N, 0.5, JL, JS, seed=1)]
    server.run()
    eng = server.engines[0]
    graphs, rows = (eng.graph, eng.graph_multi), len(eng.table.t)
    assert graphs[0] is not None
    again = [server.submit_img2img_latents(lat, STRENGTH, soft, N, 0.5, seed=s) for s in (1, 2)]
    again += [server.submit_inpaint_latents(lat, hard, N, 0.5, JL, JS, seed=s) for s in (1, 2)]
    server.run()
    assert (eng.graph, eng.graph_multi) == graphs and len(eng.table.t) == rows, "no new capture, no new rows"
    assert torch.equal(again[0].result(), first[0].result()) and torch.equal(again[2].result(), first[1].result())
    assert not torch.equal(again[1].result(), first[0].result()) and not torch.equal(again[3].result(), first[1].result())


def test_host_and_device_planes_give_the_same_result(tiny32, served):
    """exchange stages host planes through pinned memory and copies device planes directly."""
    from afldm_amd.engine import EditSlotEngine
    _, tickets = served
    eng = EditSlotEngine(tiny32[0], 2, True, 2, kinds=KINDS)
    lat, _, hard = _planes(EDITS[1][1])
    span = eng.add_schedule(_ddim().seeded_repaint_schedule(N, 0.5, JL, JS))
    start = _start(EDITS[1][1])
    eng.exchange({}, {0: (start, *span, EDITS[1][1], lat, hard), 1: (start.cuda(), *span, EDITS[1][1], lat.cuda()[0], hard.cuda()[0, 0])})
    eng.step(10)
    events = eng.exchange({0: 0, 1: 1}, {})
    for b in (0, 1):
        events[b].synchronize()
        assert torch.equal(eng.take(b), tickets[1].result()), b
    assert torch.equal(eng.cond[0].cpu(), lat[0]) and torch.equal(eng.cmask[1].cpu(), hard[0])


# ------------------------------------------------------------------------------------------------ 5. image level
def test_submit_img2img_and_submit_inpaint_from_images(tiny32):
    import torch.nn.functional as F
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.serving import SamplingServer
    from test_gpu_vae import build_vae
    vae, _, _ = build_vae(torch.float32)
    pipe = MyLDMPipeline(vae, tiny32[0], _ddim())
    pipe.set_progress_bar_config(disable=True)
    S = 16 * pipe._vae_ratio()
    g = torch.Generator().manual_seed(9)
    image = F.interpolate(torch.rand(1, 3, 8, 8, generator=g) * 2 - 1, size=(S, S), mode="bicubic", align_corners=False).clamp(-1, 1)
    cmap = torch.ones(1, 1, S, S)
    cmap[..., : S // 2 + 3] = 0.0
    mask = torch.zeros(1, 1, S, S)
    mask[..., : S // 2] = 1.0
    server = SamplingServer(pipe, 2, 2, kinds=KINDS)
    a = server.submit_img2img(image, STRENGTH, cmap, N, 0.5, seed=5)
    b = server.submit_inpaint(image, mask, N, 0.5, JL, JS, seed=6)
    c = server.submit(3, seed=7)
    server.run()
    # the latent request is the image's: encoded and pooled as the pipeline does
    with torch.no_grad():
        _, _, orig, lm = pipe._img2img_inputs(image, STRENGTH, cmap)
    lat_level = SamplingServer(pipe, 2, 2, kinds=KINDS)
    t = lat_level.submit_img2img_latents(orig, STRENGTH, lm, N, 0.5, seed=5)
    lat_level.run()
    assert torch.equal(t.result(), a.result())
    pt = server.decode([a, b, c], output_type="pt")
    assert tuple(pt.shape) == (3, 3, S, S) and pt.dtype == torch.float32 and torch.isfinite(pt).all()
    keep = (cmap == 0).expand_as(image)
    assert torch.equal(pt[0:1].cpu()[keep], image[keep]), "img2img's composite: pixels of change value 0 are the input's"
    keep = (mask == 1).expand_as(image)
    assert torch.equal(pt[1:2].cpu()[keep], image[keep]), "inpaint's composite: kept pixels are the input's"
    raw = server.decode([a, b, c], output_type="latent")
    assert torch.equal(raw.cpu(), torch.cat([a.result(), b.result(), c.result()]))
    assert torch.equal(pt[2:3], pipe._deliver(raw, "pt", True)[2:3]), "a row without a composite holds the decoder's values"
    only = server.decode([c], output_type="pt")
    assert torch.equal(only, pipe._deliver(raw[2:3], "pt", True)) and tuple(only.shape) == (1, 3, S, S)
    with pytest.raises(ValueError, match="submit_inpaint: mask"):
        server.submit_inpaint(image, mask[..., :8], seed=1)
    with pytest.raises(ValueError, match="seed"):
        server.submit_img2img(image)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(tiny32):
    from afldm_amd.engine import EditSlotEngine, SeededSlotEngine
    from afldm_amd.serving import SamplingServer
    server = SamplingServer(_ldm(tiny32[0]), 2, 2, kinds=KINDS)
    lat, soft, hard = _planes(1)
    with pytest.raises(ValueError, match="seed"):
        server.submit_img2img_latents(lat)
    with pytest.raises(ValueError, match="seed"):
        server.submit_inpaint_latents(lat, hard)
    with pytest.raises(ValueError, match="orig_latents"):
        server.submit_img2img_latents(lat[:, :3], seed=1)
    with pytest.raises(ValueError, match="change_map"):
        server.submit_img2img_latents(lat, change_map=soft[..., :8], seed=1)
    with pytest.raises(ValueError, match="latent_mask"):
        server.submit_inpaint_latents(lat, hard.expand(1, 4, 16, 16), seed=1)
    assert server._count == 0 and not server._queue[0]
    eng = server.engines[0]
    span = eng.add_schedule(_ddim().seeded_repaint_schedule(N, 0.0, JL, JS))
    before = (eng.pos.clone(), eng.cond.clone(), eng.cmask.clone())
    plain_span = eng.add_schedule(_ddim().seeded_schedule(3, 0.5))
    for bad in ((_start(1), *span, 1), (_start(1), *span, 1, lat, None), (_start(1), *span, 1, lat[:, :2], hard),
                (_start(1), *span, 1, lat, soft[..., :8]), (_start(1), *span, -1, lat, hard),
                (_start(1), *span, 1, None, None),                        # rows of an image-conditioned kind without planes
                (_start(1), *plain_span, 1, lat, hard)):                  # planes with rows that read none
        with pytest.raises(ValueError):
            eng.exchange({}, {0: bad})
    assert not eng._busy and all(torch.equal(a, b) for a, b in zip(before, (eng.pos, eng.cond, eng.cmask)))
    with pytest.raises(ValueError, match="kinds"):
        SeededSlotEngine(tiny32[0], 2, kinds=("ddim", "seeded", "seeded_sdedit"))
    seeded = SeededSlotEngine(tiny32[0], 2, row_capacity=16, temb_capacity=16)
    for refused in (_ddim().seeded_sdedit_schedule(N, STRENGTH), _ddim().seeded_repaint_schedule(N, 0.0, JL, JS)):
        with pytest.raises(NotImplementedError, match="schedules only"):
            seeded.add_schedule(refused)
    plain = SamplingServer(_ldm(tiny32[0]), 2, 2, kinds=("ddim", "seeded"))
    with pytest.raises(NotImplementedError, match="schedules only"):
        plain.submit_inpaint_latents(lat, hard, N, 0.0, JL, JS, seed=1)
    with pytest.raises(NotImplementedError, match="schedules only"):
        plain.submit_img2img_latents(lat, seed=1)
    assert EditSlotEngine.TABLE.KIND_CODES["seeded_repaint"] == 4 and SeededSlotEngine.TABLE.KIND_CODES == {"ddim": 0, "dpm": 1, "seeded": 2}
