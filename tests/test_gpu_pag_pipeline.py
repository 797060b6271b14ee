"""Perturbed-attention guidance end to end on MI355X: PAGEngine's replayed graphs against the eager loop (same generator, same
draws), pag_scale = 0 against the plain sampler, fp32 against the float64 oracle loop of tests/pag_oracle.py on the CPU oracle UNet
(1e-3, the project's bound for that comparison; the guidance itself moves the sample by more than 1e-2 there, test_pag_host.py),
that the UNet is left as it was found, the engine cache, and bf16 on the tiny and the FFHQ-size UNet.  bf16: no number fixed in
advance - pag_scale = 0 may differ from its fp32 run by 1.5x what the deterministic bf16 DDIM graph run differs from its fp32 run
over as many evaluations (`det`, the rule of test_gpu_ilvr.py / test_gpu_pano_pipeline.py), and at pag_scale = s by
1.5 (1 + 2 s) det: an error eps in each of e and e_p is at most (1 + 2 s) eps in g = e + s (e - e_p)."""
import pytest
import torch

import pag_oracle as po
from test_gpu_dpm import _run_across_a_dtype_change, build, rel_rms
from test_gpu_sde import _gens, _ldm, _same_state

pytestmark = pytest.mark.gpu

UP = ("up_blocks.1", "up_blocks.2")
N = 8


def _x(s=16, seed=3):
    return torch.randn(2, 4, s, s, generator=torch.Generator().manual_seed(seed))


def _processors(unet):
    from afldm_amd.pipelines.cross_frame_attn import get_unet_attn_processors
    return get_unet_attn_processors(unet)


@pytest.fixture(scope="module")
def tiny32():
    unet, cfg, sd = build("tiny", torch.float32)
    return unet, cfg, sd


# ------------------------------------------------------------------------------------------------ graph against the eager loop
@pytest.mark.parametrize("kind", ["cpu", "cuda", "list"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_graph_vs_eager_loop(tiny32, kind, eta):
    pipe = _ldm(tiny32[0])
    x = _x()
    kw = dict(latents=x, pag_scale=3.0, pag_applied_layers=UP, guidance_rescale=0.7, eta=eta, num_inference_steps=N)
    ga, gb, gc = _gens(kind, 11), _gens(kind, 11), _gens(kind, 11)
    a = pipe.pag_latents(generator=ga, **kw)
    assert "_engines" not in pipe.__dict__ and len(pipe._pag_engines) == 1
    (eng,) = pipe._pag_engines.values()
    assert eng.schedule.kind == "pag" and eng.x_nhwc.shape[0] == 2 * x.shape[0] and eng.lat.shape[0] == x.shape[0]
    assert eng.graph is not None and eng.branches == 1
    b = pipe.pag_latents(generator=gb, use_graph=False, **kw)
    err = rel_rms(a, b.float())
    print(f"[tiny PAG eta={eta}, {N} steps, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe.pag_latents(generator=gc, **kw))             # a seeded repeat, bit for bit
    assert len(pipe._pag_engines) == 1 and next(iter(pipe._pag_engines.values())) is eng


@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_scale_zero_is_the_plain_sampler(tiny32, eta):
    pipe = _ldm(tiny32[0])
    x = _x()
    ga, gb = _gens("cpu", 5), _gens("cpu", 5)
    a = pipe.pag_latents(latents=x, pag_scale=0.0, pag_applied_layers=UP, eta=eta, num_inference_steps=N, generator=ga)
    b = pipe(latents=x, eta=eta, num_inference_steps=N, generator=gb, output_type="latent")
    err = rel_rms(a, b)
    print(f"[tiny PAG pag_scale=0 eta={eta}, {N} steps] vs the plain sampler rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)


# ------------------------------------------------------------------------------------------------ fp32 against the oracle loop
def _oracle(tiny32, x, steps, sites, s, phi, eta, seed):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    _, cfg, sd = tiny32
    sched = ffhq_ddim_scheduler().pag_schedule(steps, eta, s, phi)
    g = torch.Generator().manual_seed(seed)
    return po.sample(sd, cfg, x, sched, sites, draw=sched.drawer(g, tuple(x.shape), torch.device("cpu"), torch.float32))


@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_fp32_against_the_oracle_loop(tiny32, phi, eta):
    pipe = _ldm(tiny32[0])
    x = _x()
    want = _oracle(tiny32, x, 4, UP, 3.0, phi, eta, 13)
    got = pipe.pag_latents(latents=x, pag_scale=3.0, pag_applied_layers=UP, guidance_rescale=phi, eta=eta, num_inference_steps=4,
                           generator=torch.Generator().manual_seed(13))
    err = rel_rms(got, want)
    plain = pipe(latents=x, eta=eta, num_inference_steps=4, generator=torch.Generator().manual_seed(13), output_type="latent")
    away = rel_rms(plain, want)
    print(f"[tiny PAG s=3 phi={phi} eta={eta}, 4 steps, {UP}] fp32 rel-RMS vs the oracle loop {err:.3e}; the plain sampler is {away:.3e} away")
    assert err <= 1e-3, err
    assert away > 1e-2, away


def test_all_seven_sites_against_the_oracle_loop(tiny32):
    from oracle import unet as ou
    pipe = _ldm(tiny32[0])
    x = _x()
    sites = tuple(ou.attention_sites(tiny32[1]))
    assert len(sites) == 7 and pipe.pag_sites(("down_blocks", "mid_block", "up_blocks")) == tuple(sorted(sites))
    want = _oracle(tiny32, x, 4, sites, 3.0, 0.0, 0.0, 1)
    got = pipe.pag_latents(latents=x, pag_scale=3.0, pag_applied_layers=("down_blocks", "mid_block", "up_blocks"), num_inference_steps=4)
    err = rel_rms(got, want)
    print(f"[tiny PAG s=3, 4 steps, all seven sites] fp32 rel-RMS vs the oracle loop {err:.3e}")
    assert err <= 1e-3, err


# ------------------------------------------------------------------------------------------------ the UNet is left as found
def test_the_unet_is_left_as_found(tiny32):
    pipe = _ldm(tiny32[0])
    x = _x()
    before = _processors(pipe.unet)
    ref = pipe(latents=x, num_inference_steps=4, output_type="latent")
    for use_graph in (True, False):
        pipe.pag_latents(latents=x, pag_applied_layers=UP, num_inference_steps=4, use_graph=use_graph)
        after = _processors(pipe.unet)
        assert after.keys() == before.keys() and all(after[k] is before[k] for k in before)
        assert torch.equal(pipe(latents=x, num_inference_steps=4, output_type="latent"), ref)
    with pytest.raises(ValueError):
        pipe.pag_latents(latents=x, pag_applied_layers=("up_blocks.1", "nowhere"), num_inference_steps=4)
    after = _processors(pipe.unet)
    assert all(after[k] is before[k] for k in before)
    assert torch.equal(pipe(latents=x, num_inference_steps=4, output_type="latent"), ref)
    # an exception inside the perturbed section puts the processors back too
    from afldm_amd.engine import pag_processors
    with pytest.raises(RuntimeError):
        with pag_processors(pipe.unet, pipe.pag_sites(UP)):
            assert any(after[k] is not p for k, p in _processors(pipe.unet).items())
            raise RuntimeError("inside")
    after = _processors(pipe.unet)
    assert all(after[k] is before[k] for k in before)


# ------------------------------------------------------------------------------------------------ engine cache
def test_engine_cache_and_refold_after_a_weight_edit():
    unet, _, _ = build("tiny", torch.float32)
    pipe = _ldm(unet)
    x, y = _x(), _x(seed=4)
    kw = dict(pag_applied_layers=UP, num_inference_steps=4)
    a = pipe.pag_latents(latents=x, pag_scale=3.0, **kw)
    (eng,) = pipe._pag_engines.values()
    graph = eng.graph
    b = pipe.pag_latents(latents=y, pag_scale=3.0, **kw)
    assert next(iter(pipe._pag_engines.values())) is eng and eng.graph is graph and not torch.equal(a, b)
    pipe.pag_latents(latents=x, pag_scale=2.0, **kw)                          # another scale: another schedule key
    (eng2,) = pipe._pag_engines.values()
    assert eng2 is not eng and eng2.sites == pipe.pag_sites(UP)
    pipe.pag_latents(latents=x, pag_scale=2.0, pag_applied_layers=("up_blocks.1",), num_inference_steps=4)      # other sites
    (eng3,) = pipe._pag_engines.values()
    assert eng3 is not eng2 and eng3.sites == pipe.pag_sites(("up_blocks.1",))
    # a weight edit: refresh_if_stale drops the graphs and the folded W_vo is formed again
    a = pipe.pag_latents(latents=x, pag_scale=3.0, **kw)
    (eng,) = pipe._pag_engines.values()
    with torch.no_grad():
        unet.up_blocks[1].attentions[0].to_v.weight.mul_(1.5)
    c = pipe.pag_latents(latents=x, pag_scale=3.0, **kw)
    assert next(iter(pipe._pag_engines.values())) is eng
    moved = rel_rms(c, a)
    fresh = pipe.pag_latents(latents=x, pag_scale=3.0, use_graph=False, **kw)
    print(f"[tiny PAG] to_v.weight * 1.5 at one site moves the sample by {moved:.3e}; graph vs eager loop after it {rel_rms(c, fresh):.2e}")
    assert moved > 1e-4 and rel_rms(c, fresh) <= 1e-5


# ------------------------------------------------------------------------------------------------ bf16
def _bf16_case(name, sites):
    u32, _, _ = build(name, torch.float32)
    u16, _, _ = build(name, torch.bfloat16)
    p32, p16 = _ldm(u32), _ldm(u16)
    x = _x(u32.config.sample_size, seed=21)
    steps = 4
    det = rel_rms(p16(latents=x, num_inference_steps=steps, output_type="latent").float(),
                  p32(latents=x, num_inference_steps=steps, output_type="latent", use_graph=False))
    kw = dict(latents=x, pag_applied_layers=sites, num_inference_steps=steps)
    graph = p16.pag_latents(pag_scale=1.0, **kw)
    assert graph.dtype == torch.bfloat16
    (eng,) = p16._pag_engines.values()
    eager = p16.pag_latents(pag_scale=1.0, use_graph=False, **kw)
    assert eng.x_nhwc.dtype == torch.bfloat16 and eng.x_nhwc.shape[0] == 4
    ge = rel_rms(graph.float(), eager.float())
    e0 = rel_rms(p16.pag_latents(pag_scale=0.0, **kw).float(), p32.pag_latents(pag_scale=0.0, **kw))
    e1 = rel_rms(graph.float(), p32.pag_latents(pag_scale=1.0, **kw))
    print(f"[{name} PAG bf16, {steps} steps, batch 2, {sites}] det {det:.3e}; pag_scale 0 vs fp32 {e0:.3e} (<= {1.5 * det:.3e}); "
          f"pag_scale 1 vs fp32 {e1:.3e} (<= {4.5 * det:.3e}); graph vs eager loop {ge:.2e}")
    return det, e0, e1, ge


@pytest.mark.parametrize("min_t", [None, 4])      # the policy's route per level, and the one launch wherever there is a kernel
def test_tiny_bf16(monkeypatch, min_t):
    from afldm_amd import ops
    if min_t is not None:
        monkeypatch.setattr(ops, "_IDENTITY_MIN_T", min_t)
    det, e0, e1, ge = _bf16_case("tiny", ("down_blocks", "mid_block", "up_blocks"))
    assert e0 <= 1.5 * det and e1 <= 1.5 * 3 * det, (det, e0, e1)
    assert ge <= 1e-5, ge


@pytest.mark.parametrize("min_t", [None, 4])
def test_ffhq_bf16(monkeypatch, min_t):
    """The sites of the 8^2, 4^2 and 2^2 levels: the token counts 64, 16 and 4 at 384 and 768 channels - on the route the policy
    picks (the two launches there) and with every level sent to the one launch."""
    from afldm_amd import ops
    if min_t is not None:
        monkeypatch.setattr(ops, "_IDENTITY_MIN_T", min_t)
    det, e0, e1, ge = _bf16_case("ffhq", ("down_blocks.2", "down_blocks.3", "mid_block"))
    assert e0 <= 1.5 * det and e1 <= 1.5 * 3 * det, (det, e0, e1)
    assert ge <= 1e-5, ge


# ------------------------------------------------------------------------------------------------ a dtype change under a live engine
def test_engine_survives_a_dtype_change():
    from afldm_amd.engine import PAGEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, _, _ = build("tiny", torch.float32)
    before = _processors(unet)
    sites, sched = _ldm(unet).pag_sites(UP), ffhq_ddim_scheduler().pag_schedule(3, 0.0, 3.0, 0.0)
    eng, said, got, fresh = _run_across_a_dtype_change(lambda: PAGEngine(unet, sched, 2, 3, sites=sites), _x())
    assert said == [True]
    assert eng.x_nhwc.dtype == torch.bfloat16 and eng.x_nhwc.shape[0] == 4 and eng.lat.shape[0] == 2
    assert eng.sites == sites
    assert torch.isfinite(got).all() and torch.equal(got, fresh)
    after = _processors(unet)
    assert after.keys() == before.keys() and all(after[k] is before[k] for k in before)
