"""Self-attention guidance end to end on MI355X (tiny UNet through test_gpu_dpm.build): SAGEngine's replayed graphs against the eager
loop (same generator, same draws), sag_scale = 0 against the plain sampler, fp32 against the float64 oracle loop of
tests/sag_oracle.py (1e-3, the project's bound for that comparison; the guidance itself moves the sample by more than 1e-2 there,
test_sag_host.py), that the UNet is left as it was found, the engine cache, and bf16 on the tiny and the FFHQ-size UNet.

The mask is a threshold, so a closed-loop comparison means something only where no mass sits on it.  THE MARGIN CONDITION: for
every closed-loop fp32 configuration the float64 oracle loop's own min |mass - 1| is at least 1e-4 (asserted on the CPU by
test_sag_host.py, and again here), and the product's recorded masses are within a quarter of that measured margin of the oracle's:
then no mask can differ, and the latents are held to the project's bounds.

bf16: no number is fixed in advance.  The bf16 eager run REPLAYS the masks of the fp32 eager run (masks=, return_masks) - a
free-running bf16 loop may legitimately threshold differently - and may differ from it by 1.5 (1 + 2 s) det, PAG's rule
(test_gpu_pag_pipeline.py): det is the deterministic bf16-vs-fp32 DDIM difference over as many UNet evaluations, measured in the
same test, and an error eps in each of e and e_d is at most (1 + 2 s) eps in g = e + s (e - e_d)."""
import pytest
import torch

import sag_oracle as so
from test_gpu_dpm import _run_across_a_dtype_change, build, rel_rms
from test_gpu_sde import _ldm, _same_state

pytestmark = pytest.mark.gpu

# a CUDA generator's draws exist on the device only; its configuration's margin is asserted on the product's recorded masses
CUDA_SEED = 1


def _processors(unet):
    from afldm_amd.pipelines.cross_frame_attn import get_unet_attn_processors
    return get_unet_attn_processors(unet)


@pytest.fixture(scope="module")
def tiny32():
    unet, cfg, sd = build("tiny", torch.float32)
    return unet, cfg, sd


def _margin(masses):
    return min(float((m.double() - 1.0).abs().min()) for m in masses)


# ------------------------------------------------------------------------------------------------ graph against the eager loop
@pytest.mark.parametrize("kind", ["cpu", "cuda", "list"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_graph_vs_eager_loop(tiny32, kind, eta):
    pipe = _ldm(tiny32[0])
    x = so.start_latents(so.GRAPH_XSEED, 2)
    kw = dict(latents=x, sag_scale=so.GRAPH_SCALE, sag_site=so.GRAPH_SITE, eta=eta, num_inference_steps=so.GRAPH_STEPS)
    seed = CUDA_SEED if kind == "cuda" else so.GRAPH_GSEED
    ga, gb, gc = (so.graph_generator(kind, seed) for _ in range(3))
    a = pipe.sag_latents(generator=ga, **kw)
    assert "_engines" not in pipe.__dict__ and len(pipe._sag_engines) == 1
    (eng,) = pipe._sag_engines.values()
    assert eng.schedule.kind == "sag" and eng.x_nhwc.shape[0] == 2 and eng.eps2.shape[0] == 4 and tuple(eng.mass.shape) == (2, 16)
    assert eng.graph is not None and eng.graph_multi is not None and eng.branches == 1
    b, masses = pipe.sag_latents(generator=gb, use_graph=False, return_masks=True, **kw)
    # the margin: the oracle loop's for CPU draws, the product's own recorded masses for device draws
    got_margin = _margin(masses)
    if kind == "cuda" and eta:
        margin = got_margin
    else:
        _, want_masses, margin = so.graph_loop(tiny32[2], tiny32[1], eta, "cpu" if kind == "cuda" else kind)
        off = max(float((m.cpu().double() - w).abs().max()) for m, w in zip(masses, want_masses))
        assert off <= margin / 4, (off, margin)
    err = rel_rms(a, b.float())
    print(f"[tiny SAG eta={eta}, {so.GRAPH_STEPS} steps, {kind} generator] margin {margin:.3e} (product's masses {got_margin:.3e}); "
          f"graph vs eager loop rel-RMS {err:.2e}")
    assert margin >= so.MARGIN, margin
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe.sag_latents(generator=gc, **kw))             # a seeded repeat, bit for bit
    assert len(pipe._sag_engines) == 1 and next(iter(pipe._sag_engines.values())) is eng
    assert float((eng.mass - masses[-1]).abs().max()) <= margin / 4         # the graph's last masses against the eager loop's


def test_engine_is_keyed_by_site_taps_and_boundary(tiny32):
    pipe = _ldm(tiny32[0])
    x = so.start_latents(so.GRAPH_XSEED, 2)
    kw = dict(latents=x, num_inference_steps=2)
    pipe.sag_latents(sag_site="mid_block", **kw)
    (eng,) = pipe._sag_engines.values()
    graph = eng.graph
    pipe.sag_latents(sag_site="mid_block.attentions.0", **kw)              # the same module: the same engine, nothing re-captured
    assert next(iter(pipe._sag_engines.values())) is eng and eng.graph is graph
    seen = [eng]
    for change in (dict(sag_site="up_blocks.1.attentions.0"), dict(sag_site="mid_block", blur_kernel_size=5),
                   dict(sag_site="mid_block", blur_sigma=2.0), dict(sag_site="mid_block", blur_boundary="circular"),
                   dict(sag_site="mid_block", sag_scale=1.0)):
        pipe.sag_latents(**dict(kw, **change))
        (e2,) = pipe._sag_engines.values()
        assert all(e2 is not s for s in seen), change
        seen.append(e2)
    assert seen[1].site == "up_blocks.1.attentions.0" and tuple(seen[1].mass.shape) == (2, 64)
    assert len(seen[2].taps) == 5 and seen[0].boundary == "reflect" and seen[4].boundary == "circular"


def test_scale_zero_is_the_plain_sampler(tiny32):
    pipe = _ldm(tiny32[0])
    x = so.start_latents(2, 2)
    for eta in (0.0, 0.7):
        ga, gb = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
        a = pipe.sag_latents(latents=x, sag_scale=0.0, sag_site="up_blocks.1.attentions.0", eta=eta, num_inference_steps=6, generator=ga)
        b = pipe(latents=x, eta=eta, num_inference_steps=6, generator=gb, output_type="latent")
        err = rel_rms(a, b)
        print(f"[tiny SAG sag_scale=0 eta={eta}, 6 steps] vs the plain sampler rel-RMS {err:.2e}")
        assert err <= 1e-5, err
        assert _same_state(ga, gb)


# ------------------------------------------------------------------------------------------------ fp32 against the oracle loop
@pytest.mark.parametrize("name", sorted(so.CLOSED_LOOPS))
def test_fp32_against_the_oracle_loop(tiny32, name):
    _, cfg, sd = tiny32
    pipe = _ldm(tiny32[0])
    site, seed, steps, B, scale, eta, gseed = so.CLOSED_LOOPS[name]
    x, want, want_masses, margin = so.closed_loop(name, sd, cfg)
    assert margin >= so.MARGIN, margin
    kw = dict(latents=x, sag_scale=scale, sag_site=site, eta=eta, num_inference_steps=steps)
    eager, masses = pipe.sag_latents(use_graph=False, return_masks=True, generator=torch.Generator().manual_seed(gseed), **kw)
    off = max(float((m.cpu().double() - w).abs().max()) for m, w in zip(masses, want_masses))
    assert len(masses) == steps and off <= margin / 4, (off, margin)      # then no mask can differ
    assert all(torch.equal(m.cpu() > 1.0, w > 1.0) for m, w in zip(masses, want_masses))
    got = pipe.sag_latents(generator=torch.Generator().manual_seed(gseed), **kw)
    err, err_eager = rel_rms(got, want), rel_rms(eager, want)
    plain = pipe(latents=x, eta=eta, num_inference_steps=steps, generator=torch.Generator().manual_seed(gseed), output_type="latent")
    away = rel_rms(plain, want)
    print(f"[tiny SAG {name}: {site}, scale {scale}, {steps} steps] oracle margin {margin:.3e}, product's masses off by {off:.2e}; "
          f"fp32 rel-RMS vs the oracle loop: graph {err:.3e}, eager {err_eager:.3e}; the plain sampler is {away:.3e} away")
    assert err <= 1e-3 and err_eager <= 1e-3, (err, err_eager)
    assert away > 1e-2, away


# ------------------------------------------------------------------------------------------------ processor hygiene
def test_the_unet_is_left_as_found(tiny32):
    from afldm_amd.engine import sag_processor
    pipe = _ldm(tiny32[0])
    x = so.start_latents(3, 2)
    before = _processors(pipe.unet)
    ref = pipe(latents=x, num_inference_steps=4, output_type="latent")
    for use_graph in (True, False):
        pipe.sag_latents(latents=x, sag_site="up_blocks.1.attentions.0", num_inference_steps=4, use_graph=use_graph)
        after = _processors(pipe.unet)
        assert after.keys() == before.keys() and all(after[k] is before[k] for k in before)
        assert torch.equal(pipe(latents=x, num_inference_steps=4, output_type="latent"), ref)
    with pytest.raises(ValueError):
        pipe.sag_latents(latents=x, sag_site="up_blocks.1", num_inference_steps=4)
    # an exception raised mid-call, inside the UNet evaluation that has the SAG processor installed
    mod = pipe.unet.up_blocks[2].attentions[0]
    original = mod.forward

    def boom(*a, **k):
        assert any(after[k] is not p for k, p in _processors(pipe.unet).items())      # the SAG processor is in place right now
        raise RuntimeError("mid-call")

    for use_graph in (False, True):
        mod.forward = boom
        try:
            with pytest.raises(RuntimeError, match="mid-call"):
                pipe.sag_latents(latents=x, sag_site="up_blocks.1.attentions.0", num_inference_steps=3, use_graph=use_graph)
        finally:
            mod.forward = original
        after = _processors(pipe.unet)
        assert all(after[k] is before[k] for k in before)
    with pytest.raises(RuntimeError):
        with sag_processor(pipe.unet, "mid_block.attentions.0"):
            raise RuntimeError("inside")
    after = _processors(pipe.unet)
    assert all(after[k] is before[k] for k in before)
    assert torch.equal(pipe(latents=x, num_inference_steps=4, output_type="latent"), ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_sites_block_output_is_the_kv_sink_routes(dtype):
    """SAGAttnProcessor's block output against AttnProcessor2_0 called with a no-op kv_sink, bit for bit, at every site of the tiny
    UNet; and the mass it reports is ops.attn_key_mass of the block's own q and k."""
    from afldm_amd import ops
    from afldm_amd.models.blocks import AttnProcessor2_0, SAGAttnProcessor
    unet, cfg, _ = build("tiny", dtype)
    g = torch.Generator().manual_seed(17)
    mods = dict(unet.named_modules())
    from oracle import unet as ou
    for site in ou.attention_sites(cfg):
        attn = mods[site]
        C = attn.to_q.weight.shape[0]
        side = {"mid_block": 4, "down_blocks.1": 8, "up_blocks.1": 8}.get(site.split(".attentions")[0], 16)      # as in the UNet
        h = (torch.randn(2, side, side, C, generator=g) * 1.5).to("cuda", dtype)
        seen = {}
        want = AttnProcessor2_0()(attn, h, kv_sink=lambda k, vt: None, qk_sink=None)
        keep = AttnProcessor2_0()(attn, h, kv_sink=lambda k, vt: None, qk_sink=lambda q, k: seen.update(q=q.clone(), k=k.clone()))
        proc = SAGAttnProcessor()
        got = proc(attn, h)
        assert torch.equal(got, want) and torch.equal(keep, want), site
        assert tuple(proc.mass.shape) == (2, side * side) and proc.mass.dtype == torch.float32
        assert torch.equal(proc.mass, ops.attn_key_mass(seen["q"], seen["k"], attn.heads, scale=attn.scale))
        given = torch.zeros(2, side * side, device="cuda")
        SAGAttnProcessor(given)(attn, h)
        assert torch.equal(given, proc.mass)                               # an engine-owned buffer is written in place


# ------------------------------------------------------------------------------------------------ bf16
def _bf16_case(name, site, scale=0.75):
    u32, _, _ = build(name, torch.float32)
    u16, _, _ = build(name, torch.bfloat16)
    p32, p16 = _ldm(u32), _ldm(u16)
    s = u32.config.sample_size
    x = torch.randn(2, 4, s, s, generator=torch.Generator().manual_seed(21))
    steps = 3
    # as many UNet evaluations as the guided run makes: 2 per step
    det = rel_rms(p16(latents=x, num_inference_steps=2 * steps, output_type="latent").float(),
                  p32(latents=x, num_inference_steps=2 * steps, output_type="latent", use_graph=False))
    kw = dict(latents=x, sag_scale=scale, sag_site=site, num_inference_steps=steps)
    graph = p16.sag_latents(**kw)
    assert graph.dtype == torch.bfloat16 and torch.isfinite(graph.float()).all()
    (eng,) = p16._sag_engines.values()
    assert eng.x_nhwc.dtype == torch.bfloat16 and eng.eps2.dtype == torch.bfloat16 and eng.mass.dtype == torch.float32
    assert torch.equal(graph, p16.sag_latents(**kw))                       # a seeded repeat, bit for bit
    ref, masses = p32.sag_latents(use_graph=False, return_masks=True, **kw)
    masks = [m > 1.0 for m in masses]
    replay = p16.sag_latents(use_graph=False, masks=masks, **kw)
    assert torch.isfinite(replay.float()).all()
    err = rel_rms(replay.float(), ref)
    bound = 1.5 * (1 + 2 * scale) * det
    masked = sum(int(m.sum()) for m in masks) / sum(m.numel() for m in masks)
    print(f"[{name} SAG bf16, {steps} steps, batch 2, {site}, scale {scale}] det {det:.3e}; bf16 on the fp32 run's masks vs fp32 "
          f"{err:.3e} (<= {bound:.3e}); {100 * masked:.0f} % of the keys masked")
    assert 0.0 < masked < 1.0
    assert err <= bound, (err, bound)


def test_tiny_bf16():
    _bf16_case("tiny", "up_blocks.2.attentions.0")


def test_ffhq_bf16():
    _bf16_case("ffhq", "up_blocks.2.attentions.0")


# ------------------------------------------------------------------------------------------------ a dtype change under a live engine
def test_engine_survives_a_dtype_change():
    from afldm_amd import ops
    from afldm_amd.engine import SAGEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, _, _ = build("tiny", torch.float32)
    before = _processors(unet)
    site, taps = _ldm(unet).sag_site_of("mid_block"), ops.gaussian_taps()
    sched = ffhq_ddim_scheduler().sag_schedule(3, 0.0, 0.75, 0.0)
    make = lambda: SAGEngine(unet, sched, 2, 3, site=site, taps=taps, boundary="reflect")
    eng, said, got, fresh = _run_across_a_dtype_change(make, so.start_latents(so.GRAPH_XSEED, 2))
    assert said == [True]
    assert eng.x_nhwc.dtype == eng.eps2.dtype == torch.bfloat16 and eng.x_nhwc.shape[0] == 2 and eng.eps2.shape[0] == 4
    assert (eng.site, eng.taps, eng.boundary) == (site, taps, "reflect")
    assert torch.isfinite(got).all() and torch.equal(got, fresh)
    after = _processors(unet)
    assert after.keys() == before.keys() and all(after[k] is before[k] for k in before)
