"""High-resolution sampling end to end on MI355X: MyLDMPipeline.hires_latents on replayed graphs (HiresEngine) against its own eager
loop (same generator, same draws), against the CPU oracle UNet driven by the float64 restatement of tests/hires_oracle.py, against
panorama_latents where the three global terms are switched off, the engine cache, scale 4, an FFHQ-size bf16 run, the pixel path
and the refusals.  Graph against eager and the reduction: rel-RMS 1e-5; fp32 against the oracle: 1e-3 (the sibling files' bounds
for the same comparisons).  bf16: no number fixed in advance - the graph run may differ from the fp32 eager loop on the same draws
by 1.5x what the deterministic bf16 DDIM graph run differs from its fp32 run over as many evaluations at as large a batch
(test_gpu_pano_pipeline's construction)."""
import pytest
import torch

import hires_oracle as ho
from test_gpu_dpm import build, rel_rms
from test_gpu_sde import _gens, _ldm, _same_state

pytestmark = pytest.mark.gpu

N = 6


@pytest.fixture(scope="module")
def tiny():
    unet, cfg, sd = build("tiny", torch.float32)
    return dict(unet=unet, cfg=cfg, sd=sd, pipe=_ldm(unet))


def base_latents(P, seed=9, S=16, C=4):
    return torch.randn(P, C, S, S, generator=torch.Generator().manual_seed(seed))


def upsampled(base, scale):
    """ref = U z0 U^T as hires_latents takes it (afldm_af_resample in fp32)."""
    from afldm_amd import ops
    z0 = ops.to_nhwc(base.cuda().float().contiguous())
    return ops.to_nchw(ops.af_resample(z0, ops.up_matrix(base.shape[-1], scale, z0.device)))


@pytest.mark.parametrize("eta,kind", [(0.0, "cpu"), (0.7, "cpu"), (0.7, "cuda"), (0.7, "list")])
def test_tiny_graph_vs_eager_loop(tiny, eta, kind):
    pipe = tiny["pipe"]
    base = base_latents(2)
    kw = dict(scale=2, stride=8, eta=eta, num_inference_steps=N)
    ga, gb, gc, gd = _gens(kind, 11), _gens(kind, 11), _gens(kind, 11), _gens(kind, 12)
    a = pipe.hires_latents(base, generator=ga, **kw)
    assert a.dtype == torch.float32 and tuple(a.shape) == (2, 4, 32, 32)
    (key,) = pipe._hires_engines
    eng = pipe._hires_engines[key]
    g, sched = eng.geometry, eng.schedule
    assert (g.oy, g.ox, g.nwin) == ((0, 8, 16), (0, 8, 16), 9) and eng.scale == 2 and eng.P == 2 and eng.branches == 1
    assert sched.kind == "hires" and len(sched.rows) == N and any(sched.draws) == (eta != 0.0)
    assert tuple(eng.lat.shape) == (26, 4, 16, 16) and tuple(eng.canvas.shape) == (2, 4, 32, 32)
    assert tuple(eng.known.shape) == tuple(eng.eps_ref.shape) == (2, 4, 32, 32) and tuple(eng.filter.shape) == (32, 32)
    assert (eng.noise is None) == (eta == 0.0) and (eta == 0.0 or tuple(eng.noise.shape) == (N, 2, 4, 32, 32))
    b = pipe.hires_latents(base, generator=gb, use_graph=False, **kw)
    err = rel_rms(a, b)
    print(f"[tiny hires 16 -> 32, stride 8, 9 + 4 windows, N={N}, eta={eta}, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe.hires_latents(base, generator=gc, **kw))                          # seeded: bit-identical
    assert pipe._hires_engines[key] is eng
    other = pipe.hires_latents(base, generator=gd, **kw)                                         # another seed: another sample
    assert rel_rms(other, a) > 1e-2


def test_tiny_vs_oracle(tiny):
    """16 -> 32, stride 16 (4 + 4 windows), N = 4, eta = 0.7: the oracle UNet on the CPU under the float64 loop, drawing the same
    noise from the same CPU generator, with the fp32 matrices the pipeline uses."""
    from oracle import unet as ou
    from afldm_amd import _lib
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = tiny["pipe"]
    base = base_latents(1, seed=4)
    got = pipe.hires_latents(base, scale=2, stride=16, eta=0.7, num_inference_steps=4, generator=torch.Generator().manual_seed(31))
    g = pipe.panorama_geometry(32, 32, 16)
    assert g.nwin == 4
    gen = torch.Generator().manual_seed(31)
    sch = ffhq_ddim_scheduler()
    sched = sch.hires_schedule(4, 0.7)
    assert any(sched.draws)
    eps_ref = torch.randn(1, 4, 32, 32, generator=gen)
    want = ho.sample(lambda w, t: ou.unet_forward(tiny["sd"], tiny["cfg"], w, t), base, _lib.filter_matrix(0, 16, 2),
                     ilvr_filter(32, 2).float(), g, 2, sched, sch.hires_start(4, 1.0), eps_ref,
                     lambda: torch.randn(1, 4, 32, 32, generator=gen))
    err = rel_rms(got, want)
    print(f"[tiny hires 16 -> 32, 4 + 4 windows, 4 evaluations, eta=0.7] fp32 rel-RMS vs the oracle loop {err:.3e}")
    assert err <= 1e-3, err


def test_tiny_switches(tiny):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = tiny["pipe"]
    base = base_latents(2, seed=5)
    kw = dict(scale=2, stride=8, num_inference_steps=N)
    # all three off: MultiDiffusion from the same noised reference (the dilated windows are evaluated, and weigh 0)
    off = pipe.hires_latents(base, cosine_scale_1=None, cosine_scale_2=None, cosine_scale_3=None,
                             generator=torch.Generator().manual_seed(1), **kw)
    k0, k1, f0 = ffhq_ddim_scheduler().hires_start(N, None)
    assert f0 == 0.0
    eps_ref = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(1))
    start = k0 * upsampled(base, 2) + k1 * eps_ref.cuda()
    pano = pipe.panorama_latents(32, 32, stride=8, num_inference_steps=N, latents=start)
    err = rel_rms(off, pano)
    print(f"[tiny hires 16 -> 32, all three cosine scales None] vs panorama_latents from the noised reference rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    # each term does something
    full = pipe.hires_latents(base, generator=torch.Generator().manual_seed(1), **kw)
    for name in ("cosine_scale_1", "cosine_scale_2", "cosine_scale_3"):
        one_off = pipe.hires_latents(base, generator=torch.Generator().manual_seed(1), **dict(kw, **{name: None}))
        d = rel_rms(one_off, full)
        print(f"[tiny hires 16 -> 32] {name}=None against the default: rel-RMS {d:.2e}")
        if name == "cosine_scale_2":
            assert d > 1e-2, d                                            # the global path does something
        else:
            assert d > 0.0


def test_tiny_engine_cache(tiny):
    pipe = tiny["pipe"]
    pipe(batch_size=1, num_inference_steps=2, output_type="latent", generator=torch.Generator().manual_seed(0))   # a base sample's engine
    plain = dict(pipe._engines)
    kw = dict(scale=2, stride=8, num_inference_steps=N)
    b1, b2 = base_latents(1, seed=6), base_latents(1, seed=7)

    def run(base, seed=2, **over):
        return pipe.hires_latents(base, generator=torch.Generator().manual_seed(seed), **dict(kw, **over))
    a = run(b1)
    (key,) = pipe._hires_engines
    eng = pipe._hires_engines[key]
    graphs = (eng.graph, eng.graph_multi)
    assert graphs[0] is not None and graphs[1] is not None               # the 1-step and the steps_per_graph-step graph
    b = run(b2)                                                          # another base image: the same engine, no recapture
    c = run(b1, seed=3)                                                  # ... another seed likewise
    assert pipe._hires_engines[key] is eng and (eng.graph, eng.graph_multi) == graphs
    assert rel_rms(b, a) > 1e-2 and rel_rms(c, a) > 1e-2 and rel_rms(b, run(b2, use_graph=False)) <= 1e-5
    assert torch.equal(run(b1), a)                                       # ... and back
    run(b1, stride=16)                                                   # another stride: another geometry replaces the entry
    (key2,) = pipe._hires_engines
    eng2 = pipe._hires_engines[key2]
    assert key2 != key and eng2 is not eng and eng2.geometry.nwin == 4 and tuple(eng2.lat.shape) == (8, 4, 16, 16)
    run(b1, stride=16, scale=4)                                          # ... and so does another scale
    (key3,) = pipe._hires_engines
    eng3 = pipe._hires_engines[key3]
    assert key3 != key2 and eng3 is not eng2 and eng3.scale == 4 and tuple(eng3.lat.shape) == (32, 4, 16, 16)
    assert pipe._engines == plain and all(pipe._engines[k] is plain[k] for k in plain)          # the plain sampler's cache is left alone
    from afldm_amd.engine import DenoiseEngine, HiresEngine, PanoramaEngine
    sched = pipe.scheduler.hires_schedule(N)
    g = pipe.panorama_geometry(32, 32, 8)
    with pytest.raises(NotImplementedError):                              # a "hires" schedule is HiresEngine's alone
        DenoiseEngine(tiny["unet"], sched, 13, N)
    with pytest.raises(NotImplementedError):
        PanoramaEngine(tiny["unet"], sched, 9, N, geometry=g)
    with pytest.raises(NotImplementedError):                              # ... and it takes no other
        HiresEngine(tiny["unet"], pipe.scheduler.panorama_schedule(N), 13, N, geometry=g, scale=2)
    for batch, geom, scale in ((9, g, 2), (13, g, 3), (13, pipe.panorama_geometry(32, 40, 8), 2), (13, None, 2)):
        with pytest.raises(ValueError):
            HiresEngine(tiny["unet"], sched, batch, N, geometry=geom, scale=scale)
    # the engine's own checks of known=
    x = torch.zeros(1, 4, 32, 32)
    with pytest.raises(ValueError):
        eng3.run(torch.zeros(1, 4, 64, 64), draw=lambda: x)
    with pytest.raises(ValueError):
        eng3.run(torch.zeros(1, 4, 64, 64), draw=lambda: x, known=(x, torch.zeros(1, 4, 64, 64)))


def test_tiny_scale_four(tiny):
    """16 -> 64: the largest canvas the update takes, 16 + 16 windows."""
    pipe = tiny["pipe"]
    base = base_latents(1, seed=8)
    kw = dict(scale=4, stride=16, eta=0.7, num_inference_steps=3)
    a = pipe.hires_latents(base, generator=torch.Generator().manual_seed(5), **kw)
    (eng,) = pipe._hires_engines.values()
    assert tuple(a.shape) == (1, 4, 64, 64) and torch.isfinite(a).all() and tuple(eng.lat.shape) == (32, 4, 16, 16)
    b = pipe.hires_latents(base, generator=torch.Generator().manual_seed(5), use_graph=False, **kw)
    err = rel_rms(a, b)
    print(f"[tiny hires 16 -> 64, stride 16, 16 + 16 windows, eta=0.7] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err


# ------------------------------------------------------------------------------------------------ FFHQ size, bf16
def test_ffhq_bf16_graph_vs_fp32_eager_and_the_refusals_at_that_size(monkeypatch):
    from afldm_amd.schedulers.schedule import Schedule
    from afldm_amd.utils import randn_tensor
    u32, _, _ = build("ffhq", torch.float32)
    u16, _, _ = build("ffhq", torch.bfloat16)
    p32, p16 = _ldm(u32), _ldm(u16)
    s = u32.config.sample_size
    evals = 4
    kw = dict(scale=2, stride=s // 2, eta=0.7, num_inference_steps=evals)
    gen = torch.Generator().manual_seed(21)
    plain = torch.randn(13, 4, s, s, generator=gen)                       # as many planes as the canvas has windows
    base = torch.randn(1, 4, s, s, generator=gen).bfloat16().float()
    # the yardstick: the deterministic bf16 DDIM graph run against its fp32 run over as many evaluations
    det = rel_rms(p16(latents=plain, num_inference_steps=evals, output_type="latent").float(),
                  p32(latents=plain, num_inference_steps=evals, output_type="latent", use_graph=False))
    # the fp32 eager loop on the draws of the bf16 run: a bf16 model draws its noise in bf16
    with monkeypatch.context() as mp:
        mp.setattr(Schedule, "draw_noise", lambda self, shape, generator, device, model_dtype:
                   randn_tensor(shape, generator=generator, device=device, dtype=torch.bfloat16))
        want = p32.hires_latents(base, generator=torch.Generator().manual_seed(41), use_graph=False, **kw)
    got = p16.hires_latents(base, generator=torch.Generator().manual_seed(41), **kw)
    (eng,) = p16._hires_engines.values()
    assert eng.geometry.nwin == 9 and tuple(eng.lat.shape) == (13, 4, s, s) and eng.x_nhwc.dtype == torch.bfloat16
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 4, 2 * s, 2 * s) and torch.isfinite(got).all()
    err = rel_rms(got, want)
    print(f"[FFHQ hires {s} -> {2 * s}, stride {s // 2}, 9 + 4 windows, eta=0.7, {evals} evaluations] bf16 graph rel-RMS vs the fp32 eager "
          f"loop {err:.3e}; bf16 DDIM graph vs fp32, {evals} steps, batch 13: {det:.3e}")
    assert err <= 1.5 * det, (err, det)
    # 4 x 32 = 128 latents: beyond the one-workgroup plane
    with pytest.raises(ValueError, match="64"):
        p16.hires_latents(base, scale=4)
    assert len(p16._hires_engines) == 1 and next(iter(p16._hires_engines.values())) is eng


# ------------------------------------------------------------------------------------------------ pixels, refusals
def test_tiny_pixel_path(tiny):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from test_gpu_vae import build_vae
    vae, _, _ = build_vae(torch.float32)
    pipe = MyLDMPipeline(vae, tiny["unet"], ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    r = pipe._vae_ratio()

    def run(**over):
        return pipe.hires(**dict(dict(batch_size=2, scale=2, num_inference_steps=2, generator=torch.Generator().manual_seed(3)), **over))
    pt = run(output_type="pt")
    assert pt.dtype == torch.float32 and tuple(pt.shape) == (2, 3, r * 32, r * 32) and torch.isfinite(pt).all()
    canvas = run(output_type="latent")
    assert canvas.dtype == torch.float32 and tuple(canvas.shape) == (2, 4, 32, 32)
    assert torch.equal(pt, pipe.decode_panorama(canvas, pipe.panorama_geometry(32, 32, 8)))
    # given base latents: no base sample is drawn
    base = base_latents(2, seed=2)
    given = run(base_latents=base, output_type="latent")
    assert torch.equal(given, pipe.hires_latents(base, num_inference_steps=2, generator=torch.Generator().manual_seed(3)))
    # a stride in pixels
    wide = run(base_latents=base, stride=16 * r, output_type="latent")
    (eng,) = pipe._hires_engines.values()
    assert eng.geometry.nwin == 4 and tuple(wide.shape) == (2, 4, 32, 32)
    out = run(base_latents=base)
    assert len(out.images) == 2 and out.images[0].size == (r * 32, r * 32)
    with pytest.raises(ValueError):
        run(stride=r + 1)
    with pytest.raises(NotImplementedError):
        tiny["pipe"].hires()                                              # no VAE


def test_refusals(tiny):
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    pipe = _ldm(tiny["unet"])
    base = base_latents(1)
    for scale in (1, 0, 1.5):
        with pytest.raises(ValueError, match="scale"):
            pipe.hires_latents(base, scale=scale)
    with pytest.raises(ValueError, match="64"):
        pipe.hires_latents(base, scale=5)                                 # 80 latents
    for bad in (base[:, :3], base[..., :8], base[0]):
        with pytest.raises(ValueError, match="base_latents"):
            pipe.hires_latents(bad)
    assert "_hires_engines" not in pipe.__dict__
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    with pytest.raises(NotImplementedError):
        pipe.hires_latents(base)
    with pytest.raises(NotImplementedError):
        pipe.hires()
