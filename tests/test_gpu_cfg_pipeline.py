"""Classifier-free guidance end to end on MI355X: CFGEngine's replayed graphs against the eager loop (same generator, same draws),
relabelling on the same graphs, guidance_scale = 1 against a hand-written conditional loop, fp32 against the float64 oracle loop of
tests/cfg_oracle.py on the CPU oracle UNet (1e-3, the project's bound for that comparison; the guidance itself moves the sample by
more than 1e-2 there, test_cfg_host.py), the engine cache, the refusals, and bf16 on the tiny and the FFHQ-size UNet.  bf16: no
number fixed in advance - the rule and derivation of test_gpu_pag_pipeline.py's docstring with s = w - 1: guidance_scale = 1 may
differ from its fp32 run by 1.5x what the deterministic bf16 DDIM graph run of the unconditional model of the same weights
differs from its fp32 run over as many evaluations (`det`), and at guidance_scale = w by 1.5 (1 + 2 (w - 1)) det: an error eps in
each of e_c and e_u is at most (1 + 2 (w - 1)) eps in g = e_c + (w - 1) (e_c - e_u)."""
import pytest
import torch

import cfg_oracle as co
from test_gpu_dpm import _run_across_a_dtype_change, build, dpm, rel_rms
from test_gpu_sde import _gens, _ldm, _same_state

pytestmark = pytest.mark.gpu

N = 8
LABELS = [0, 3]


def _x(s=16, seed=3):
    return torch.randn(2, 4, s, s, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def cond32():
    return co.build_cond(torch.float32)


# ------------------------------------------------------------------------------------------------ graph against the eager loop
@pytest.mark.parametrize("kind", ["cpu", "cuda", "list"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_graph_vs_eager_loop(cond32, kind, eta):
    pipe = _ldm(cond32[0])
    x = _x()
    kw = dict(latents=x, guidance_scale=3.0, guidance_rescale=0.7, eta=eta, num_inference_steps=N)
    ga, gb, gc = _gens(kind, 11), _gens(kind, 11), _gens(kind, 11)
    a = pipe.cfg_latents(LABELS, generator=ga, **kw)
    assert "_engines" not in pipe.__dict__ and len(pipe._cfg_engines) == 1
    (eng,) = pipe._cfg_engines.values()
    assert eng.schedule.kind == "cfg" and eng.x_nhwc.shape[0] == 2 * x.shape[0] and eng.lat.shape[0] == x.shape[0]
    assert eng.class_rows.shape[0] == eng.act.shape[0] == eng.temb_rows.shape[0] == 2 * x.shape[0]
    assert tuple(eng.emb_table.shape) == (N, eng.class_rows.shape[1])
    assert eng.graph is not None and eng.branches == 1 and eng.guided
    b = pipe.cfg_latents(LABELS, generator=gb, use_graph=False, **kw)
    err = rel_rms(a, b.float())
    print(f"[tiny CFG w=3 phi=0.7 eta={eta}, {N} steps, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe.cfg_latents(LABELS, generator=gc, **kw))          # a seeded repeat, bit for bit
    assert len(pipe._cfg_engines) == 1 and next(iter(pipe._cfg_engines.values())) is eng


def test_relabelling_replays_the_same_graphs(cond32):
    pipe = _ldm(cond32[0])
    x = _x()
    kw = dict(latents=x, guidance_scale=3.0, num_inference_steps=4)
    a = pipe.cfg_latents([0, 3], **kw)
    (eng,) = pipe._cfg_engines.values()
    graph, multi, rows_at = eng.graph, eng.graph_multi, eng.class_rows.data_ptr()
    b = pipe.cfg_latents([2, 1], **kw)
    assert next(iter(pipe._cfg_engines.values())) is eng and eng.graph is graph and eng.graph_multi is multi
    assert eng.class_rows.data_ptr() == rows_at
    assert not torch.equal(a, b)
    fresh = _ldm(cond32[0])
    assert torch.equal(b, fresh.cfg_latents([2, 1], **kw))                       # a newly built engine: the same bits
    assert next(iter(fresh._cfg_engines.values())) is not eng
    assert torch.equal(a, pipe.cfg_latents([0, 3], **kw))                        # and back
    c = pipe.cfg_latents([2, 1], null_label=0, **kw)                             # another null row: data too
    assert eng.graph is graph and not torch.equal(c, b)
    assert torch.equal(c, fresh.cfg_latents([2, 1], null_label=0, **kw))


@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_scale_one_evaluates_b_rows_and_is_the_conditional_sampler(cond32, eta):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = cond32[0]
    pipe = _ldm(unet)
    x = _x()
    ga, gb = _gens("cpu", 5), _gens("cpu", 5)
    a = pipe.cfg_latents(LABELS, latents=x, guidance_scale=1.0, eta=eta, num_inference_steps=N, generator=ga)
    (eng,) = pipe._cfg_engines.values()
    assert eng.x_nhwc.shape[0] == x.shape[0] and eng.class_rows.shape[0] == x.shape[0] and not eng.guided
    assert eng.schedule.kind == ("sde" if eta else "ddim")
    sched = ffhq_ddim_scheduler()
    sched.set_timesteps(N)
    z = x.cuda()
    for t in sched._timesteps_host:                                               # unet.forward with labels, then the plain update
        eps = unet(z, t, class_labels=LABELS).sample
        z = sched.step(eps, t, z, eta=eta, generator=gb).prev_sample
    err = rel_rms(a, z)
    print(f"[tiny CFG w=1 eta={eta}, {N} steps] vs a loop of unet.forward(x, t, labels) and scheduler.step rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    e = pipe.cfg_latents(LABELS, latents=x, guidance_scale=1.0, eta=eta, num_inference_steps=N, generator=_gens("cpu", 5),
                         use_graph=False)
    assert rel_rms(a, e) <= 1e-5


# ------------------------------------------------------------------------------------------------ fp32 against the oracle loop
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_fp32_against_the_oracle_loop(cond32, phi, eta):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, cfg, sd, table = cond32
    pipe = _ldm(unet)
    x = _x()
    sched = ffhq_ddim_scheduler().cfg_schedule(4, eta, 3.0, phi)
    g = torch.Generator().manual_seed(13)
    want = co.sample(sd, cfg, x, sched, table[LABELS], table[[co.K - 1] * 2],
                     draw=sched.drawer(g, tuple(x.shape), torch.device("cpu"), torch.float32))
    got = pipe.cfg_latents(LABELS, latents=x, guidance_scale=3.0, guidance_rescale=phi, eta=eta, num_inference_steps=4,
                           generator=torch.Generator().manual_seed(13))
    err = rel_rms(got, want)
    one = pipe.cfg_latents(LABELS, latents=x, guidance_scale=1.0, eta=eta, num_inference_steps=4,
                           generator=torch.Generator().manual_seed(13))
    away = rel_rms(one, want)
    print(f"[tiny CFG w=3 phi={phi} eta={eta}, 4 steps, labels {LABELS}] fp32 rel-RMS vs the oracle loop {err:.3e}; the w = 1 sample is {away:.3e} away")
    assert err <= 1e-3, err
    assert away > 1e-2, away


def test_identity_rows_and_null_embedding(cond32):
    """An 'identity' model fed the table's rows, with the null row as null_embedding, is the Embedding model's run bit for bit."""
    unet, _, _, table = cond32
    ident, _, _, _ = co.build_cond(torch.float32, class_embed_type="identity")
    x = _x()
    kw = dict(latents=x, guidance_scale=3.0, guidance_rescale=0.7, num_inference_steps=4)
    a = _ldm(unet).cfg_latents(LABELS, **kw)
    pi = _ldm(ident)
    assert torch.equal(pi.cfg_latents(table[LABELS], null_embedding=table[co.K - 1], **kw), a)
    assert torch.equal(pi.cfg_latents(table[LABELS], null_embedding=table[co.K - 1], use_graph=False, **kw),
                       _ldm(unet).cfg_latents(LABELS, use_graph=False, **kw))
    zero = pi.cfg_latents(table[LABELS], **kw)                                   # default: zeros
    assert not torch.equal(zero, a)
    with pytest.raises(ValueError):
        pi.cfg_latents(table[LABELS], null_label=0, **kw)


# ------------------------------------------------------------------------------------------------ engine cache
def test_engine_cache_and_a_table_edit():
    unet, _, _, _ = co.build_cond(torch.float32)
    pipe = _ldm(unet)
    x = _x()
    kw = dict(latents=x, num_inference_steps=4)
    a = pipe.cfg_latents(LABELS, guidance_scale=3.0, **kw)
    (eng,) = pipe._cfg_engines.values()
    pipe.cfg_latents(LABELS, guidance_scale=2.0, **kw)                            # another scale: another schedule key
    (eng2,) = pipe._cfg_engines.values()
    assert eng2 is not eng and eng2.guided
    pipe.cfg_latents(LABELS, guidance_scale=1.0, **kw)
    (eng3,) = pipe._cfg_engines.values()
    assert eng3 is not eng2 and not eng3.guided
    # an in-place edit of the class table: the rows are embedded per call, and refresh_if_stale notices the model moved
    a = pipe.cfg_latents(LABELS, guidance_scale=3.0, **kw)
    (eng,) = pipe._cfg_engines.values()
    with torch.no_grad():
        unet.class_embedding.weight.mul_(1.5)
    c = pipe.cfg_latents(LABELS, guidance_scale=3.0, **kw)
    assert next(iter(pipe._cfg_engines.values())) is eng
    moved = rel_rms(c, a)
    fresh = pipe.cfg_latents(LABELS, guidance_scale=3.0, use_graph=False, **kw)
    # and an edit of time_embedding, which emb_table is made from
    with torch.no_grad():
        unet.time_embedding.linear_2.bias.add_(0.25)
    d = pipe.cfg_latents(LABELS, guidance_scale=3.0, **kw)
    fresh_d = pipe.cfg_latents(LABELS, guidance_scale=3.0, use_graph=False, **kw)
    print(f"[tiny CFG] class table * 1.5 moves the sample by {moved:.3e}; graph vs eager loop after it {rel_rms(c, fresh):.2e}; "
          f"linear_2.bias + 0.25 moves it by {rel_rms(d, c):.3e}; graph vs eager loop after it {rel_rms(d, fresh_d):.2e}")
    assert moved > 1e-4 and rel_rms(c, fresh) <= 1e-5
    assert rel_rms(d, c) > 1e-4 and rel_rms(d, fresh_d) <= 1e-5


# ------------------------------------------------------------------------------------------------ bf16
def _bf16_case(name):
    u32, _, _, _ = co.build_cond(torch.float32, name=name)
    u16, _, _, _ = co.build_cond(torch.bfloat16, name=name)
    q32, _, _ = build(name, torch.float32)                                       # the unconditional model of the same weights: det
    q16, _, _ = build(name, torch.bfloat16)
    x = _x(u32.config.sample_size, seed=21)
    steps = 4
    det = rel_rms(_ldm(q16)(latents=x, num_inference_steps=steps, output_type="latent").float(),
                  _ldm(q32)(latents=x, num_inference_steps=steps, output_type="latent", use_graph=False))
    del q32, q16
    p32, p16 = _ldm(u32), _ldm(u16)
    kw = dict(latents=x, num_inference_steps=steps)
    graph = p16.cfg_latents(LABELS, guidance_scale=2.0, **kw)
    assert graph.dtype == torch.bfloat16
    (eng,) = p16._cfg_engines.values()
    assert eng.x_nhwc.dtype == eng.class_rows.dtype == eng.act.dtype == eng.emb_table.dtype == torch.bfloat16
    assert eng.x_nhwc.shape[0] == 4
    eager = p16.cfg_latents(LABELS, guidance_scale=2.0, use_graph=False, **kw)
    ge = rel_rms(graph.float(), eager.float())
    e1 = rel_rms(p16.cfg_latents(LABELS, guidance_scale=1.0, **kw).float(), p32.cfg_latents(LABELS, guidance_scale=1.0, **kw))
    e2 = rel_rms(graph.float(), p32.cfg_latents(LABELS, guidance_scale=2.0, **kw))
    print(f"[{name} CFG bf16, {steps} steps, batch 2] det {det:.3e}; w = 1 vs fp32 {e1:.3e} (<= {1.5 * det:.3e}); "
          f"w = 2 vs fp32 {e2:.3e} (<= {4.5 * det:.3e}); graph vs eager loop {ge:.2e}")
    return det, e1, e2, ge


@pytest.mark.parametrize("name", ["tiny", "ffhq"])
def test_bf16(name):
    det, e1, e2, ge = _bf16_case(name)
    assert e1 <= 1.5 * det and e2 <= 1.5 * 3 * det, (det, e1, e2)
    assert ge <= 1e-5, ge


# ------------------------------------------------------------------------------------------------ a dtype change under a live engine
def test_engine_survives_a_dtype_change():
    from afldm_amd.engine import CFGEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, _, _, table = co.build_cond(torch.float32)
    sched = ffhq_ddim_scheduler().cfg_schedule(3, 0.0, 3.0, 0.0)
    rows = table[LABELS + [co.K - 1] * 2].cuda()

    def make():
        eng = CFGEngine(unet, sched, 2, 3, guided=True)
        eng.set_class_rows(rows)
        return eng
    eng, said, got, fresh = _run_across_a_dtype_change(make, _x())
    assert said == [True]
    assert eng.x_nhwc.dtype == eng.class_rows.dtype == eng.emb_table.dtype == torch.bfloat16
    assert eng.x_nhwc.shape[0] == 4 and eng.lat.shape[0] == 2
    assert torch.isfinite(got).all() and torch.equal(got, fresh)


# ------------------------------------------------------------------------------------------------ refusals
def test_other_engines_refuse_the_conditional_unet(cond32):
    from afldm_amd import engine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = cond32[0]
    s = ffhq_ddim_scheduler()
    plain, sde, pag, sag = s.schedule(3), s.stochastic_schedule(3, 0.7), s.pag_schedule(3), s.sag_schedule(3)
    makes = [lambda: engine.DenoiseEngine(unet, plain, 2, 3), lambda: engine.DenoiseEngine(unet, sde, 2, 3),
             lambda: engine.PAGEngine(unet, pag, 2, 3, sites=("mid_block.attentions.0",)),
             lambda: engine.SAGEngine(unet, sag, 2, 3, site="mid_block.attentions.0", taps=(1.0,), boundary="reflect"),
             lambda: engine.SlotEngine(unet, 2), lambda: engine.PicardEngine(unet, plain, 2, 3, window=2)]
    for make in makes:
        with pytest.raises(ValueError, match="class-conditional"):
            make()
    pipe = _ldm(unet)
    for call in (lambda: pipe(latents=_x(), num_inference_steps=3, output_type="latent"),
                 lambda: pipe(latents=_x(), num_inference_steps=3, eta=0.7, output_type="latent"),
                 lambda: pipe.pag_latents(latents=_x(), num_inference_steps=3)):
        with pytest.raises(ValueError):
            call()
    # and CFGEngine refuses what it cannot run: an unconditional UNet, a kind that does not match `guided`
    q, _, _ = build("tiny", torch.float32)
    with pytest.raises(ValueError):
        engine.CFGEngine(q, s.cfg_schedule(3), 2, 3, guided=True)
    with pytest.raises(ValueError):
        engine.CFGEngine(unet, s.cfg_schedule(3), 2, 3, guided=False)
    with pytest.raises(ValueError):
        engine.CFGEngine(unet, plain, 2, 3, guided=True)
    with pytest.raises(NotImplementedError):
        engine.CFGEngine(unet, pag, 2, 3, guided=False)
    eng = engine.CFGEngine(unet, plain, 2, 3, guided=False)
    with pytest.raises(ValueError):
        eng.run(_x())                                                             # no class rows yet
    with pytest.raises(ValueError):
        eng.run(_x(), known=torch.zeros(4, eng.class_rows.shape[1]))              # 2 B rows for an engine of B


def test_the_dpm_scheduler_is_refused(cond32):
    pipe = _ldm(cond32[0])
    pipe.scheduler = dpm()
    for call in (pipe.cfg_latents, pipe.cfg):
        with pytest.raises(NotImplementedError, match="classifier-free guidance"):
            call(LABELS, latents=_x(), num_inference_steps=2)
