"""MultiDiffusion panoramas end to end on MI355X: MyLDMPipeline.panorama_latents on replayed graphs (PanoramaEngine) against its own
eager loop (same generator, same draws), against the plain sampler where the canvas is one window, against the CPU oracle UNet
driven by the float64 restatement of tests/pano_oracle.py, under a roll of a circular canvas, the engine cache, an FFHQ-size bf16
run, and the pixel path.  Graph against eager and the roll: rel-RMS 1e-5; fp32 against the oracle: 1e-3 (tests/test_gpu_sde.py's and
test_gpu_ilvr.py's bounds for the same comparisons).  bf16: no number fixed in advance - the graph run may differ from the fp32
eager loop on the same draws by 1.5x what the deterministic bf16 DDIM graph run differs from its fp32 run over as many
evaluations."""
import pytest
import torch

import pano_oracle as po
from test_gpu_dpm import _run_across_a_dtype_change, build, rel_rms
from test_gpu_sde import _gens, _ldm, _same_state

pytestmark = pytest.mark.gpu

N = 8


@pytest.fixture(scope="module")
def tiny():
    unet, cfg, sd = build("tiny", torch.float32)
    return dict(unet=unet, cfg=cfg, sd=sd, pipe=_ldm(unet))


@pytest.mark.parametrize("eta,kind", [(0.0, "cpu"), (0.7, "cpu"), (0.7, "cuda"), (0.7, "list")])
def test_tiny_graph_vs_eager_loop(tiny, eta, kind):
    pipe = tiny["pipe"]
    kw = dict(stride=8, eta=eta, num_inference_steps=N, batch_size=2)
    ga, gb, gc, gd = (_gens(kind, 11) for _ in range(4))
    a = pipe.panorama_latents(16, 40, generator=ga, **kw)
    assert a.dtype == torch.float32 and tuple(a.shape) == (2, 4, 16, 40)
    (key,) = pipe._pano_engines
    eng = pipe._pano_engines[key]
    g = eng.geometry
    assert (g.oy, g.ox, g.nwin) == ((0,), (0, 8, 16, 24), 4) and eng.schedule.kind == "pano" and eng.branches == 1
    assert tuple(eng.lat.shape) == (8, 4, 16, 16) and tuple(eng.canvas.shape) == (2, 4, 16, 40)
    assert (eng.noise is None) if eta == 0.0 else (tuple(eng.noise.shape) == (N, 2, 4, 16, 40))
    assert "_engines" not in pipe.__dict__ or key not in pipe._engines
    b = pipe.panorama_latents(16, 40, generator=gb, use_graph=False, **kw)
    err = rel_rms(a, b)
    print(f"[tiny panorama 16 x 40, stride 8, N={N}, eta={eta}, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe.panorama_latents(16, 40, generator=gc, **kw))                      # seeded: bit-identical
    assert pipe._pano_engines[key] is eng
    if eta != 0.0:
        det = pipe.panorama_latents(16, 40, generator=gd, **dict(kw, eta=0.0))                    # the same start canvas, no noise
        assert rel_rms(a, det) > 1e-2


def test_tiny_single_window_is_the_plain_sampler(tiny):
    pipe = tiny["pipe"]
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    for eta in (0.0, 0.7):
        a = pipe.panorama_latents(16, 16, eta=eta, num_inference_steps=N, latents=x, generator=torch.Generator().manual_seed(1))
        b = pipe(latents=x, eta=eta, num_inference_steps=N, generator=torch.Generator().manual_seed(1), output_type="latent")
        err = rel_rms(a, b)
        print(f"[tiny panorama 16 x 16 = one window, eta={eta}] vs the plain sampler rel-RMS {err:.2e}")
        assert err <= 1e-5, err
    with pytest.raises(ValueError):
        pipe.panorama_latents(16, 40, latents=x)                          # a start canvas of another shape
    with pytest.raises(ValueError):
        pipe.panorama_latents(8, 40)                                      # a canvas smaller than the window


def test_tiny_vs_oracle(tiny):
    """16 x 24 canvas, stride 8, 4 steps, eta = 0.7: the oracle UNet on the CPU under the float64 loop, drawing the same noise from
    the same CPU generator."""
    from oracle import unet as ou
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = tiny["pipe"]
    x = torch.randn(1, 4, 16, 24, generator=torch.Generator().manual_seed(4))
    got = pipe.panorama_latents(16, 24, stride=8, eta=0.7, num_inference_steps=4, latents=x, generator=torch.Generator().manual_seed(31))
    g = pipe.panorama_geometry(16, 24, 8)
    assert g.ox == (0, 8)
    gen = torch.Generator().manual_seed(31)
    want = po.sample(lambda w, t: ou.unet_forward(tiny["sd"], tiny["cfg"], w, t), x, g, ffhq_ddim_scheduler().panorama_schedule(4, 0.7),
                     lambda: torch.randn(x.shape, generator=gen))
    err = rel_rms(got, want)
    print(f"[tiny panorama 16 x 24, 4 steps, eta=0.7] fp32 rel-RMS vs the oracle loop {err:.3e}")
    assert err <= 1e-3, err


def test_tiny_circular_canvas_commutes_with_a_roll_by_the_stride(tiny):
    pipe = tiny["pipe"]
    x = torch.randn(1, 4, 16, 32, generator=torch.Generator().manual_seed(5))
    kw = dict(stride=8, circular=True, num_inference_steps=N)
    a = pipe.panorama_latents(16, 32, latents=x, **kw)
    (eng,) = pipe._pano_engines.values()
    assert eng.geometry.wrap_x and eng.geometry.ox == (0, 8, 16, 24)
    b = pipe.panorama_latents(16, 32, latents=x.roll(8, -1), **kw)
    err = rel_rms(b, a.roll(8, -1))
    print(f"[tiny circular panorama 16 x 32, stride 8] roll by 8: rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    # the seam is sampled like any other column: not circular, the same start gives another canvas
    assert rel_rms(pipe.panorama_latents(16, 32, latents=x, **dict(kw, circular=False)), a) > 1e-3


def test_tiny_engine_cache(tiny):
    pipe = tiny["pipe"]
    kw = dict(stride=8, num_inference_steps=N)
    x1, x2 = (torch.randn(1, 4, 16, 40, generator=torch.Generator().manual_seed(s)) for s in (6, 7))
    a = pipe.panorama_latents(16, 40, latents=x1, **kw)
    (key,) = pipe._pano_engines
    eng = pipe._pano_engines[key]
    graphs = (eng.graph, eng.graph_multi)
    assert graphs[0] is not None
    b = pipe.panorama_latents(16, 40, latents=x2, **kw)                   # a second canvas: the same engine, no recapture
    assert pipe._pano_engines[key] is eng and (eng.graph, eng.graph_multi) == graphs
    assert rel_rms(b, a) > 1e-2 and rel_rms(b, pipe.panorama_latents(16, 40, latents=x2, use_graph=False, **kw)) <= 1e-5
    pipe.panorama_latents(16, 32, latents=x1[..., :32], **kw)             # another width: another geometry replaces the entry
    (key2,) = pipe._pano_engines
    eng2 = pipe._pano_engines[key2]
    assert key2 != key and eng2 is not eng and eng2.geometry.Wc == 32 and not eng2.geometry.wrap_x
    pipe.panorama_latents(16, 32, latents=x1[..., :32], circular=True, **kw)
    (key3,) = pipe._pano_engines
    assert key3 != key2                                                    # ... and so does the same width with a wrapping axis
    assert pipe._pano_engines[key3] is not eng2 and pipe._pano_engines[key3].geometry == pipe.panorama_geometry(16, 32, 8, True)
    from afldm_amd.engine import DenoiseEngine
    with pytest.raises(NotImplementedError):                              # the plain engine has no canvas
        DenoiseEngine(tiny["unet"], pipe.scheduler.panorama_schedule(N, 0.0), 4, N)


# ------------------------------------------------------------------------------------------------ a dtype change under a live engine
def test_tiny_engine_survives_a_dtype_change():
    from afldm_amd.engine import PanoramaEngine
    from afldm_amd.pipelines.cross_frame_attn import get_unet_attn_processors
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, _, _ = build("tiny", torch.float32)
    before = get_unet_attn_processors(unet)
    geom, sched = _ldm(unet).panorama_geometry(16, 24, 8), ffhq_ddim_scheduler().panorama_schedule(3, 0.0)
    x = torch.randn(1, 4, 16, 24, generator=torch.Generator().manual_seed(4))
    eng, said, got, fresh = _run_across_a_dtype_change(lambda: PanoramaEngine(unet, sched, geom.nwin, 3, geometry=geom), x)
    assert said == [True]
    assert eng.x_nhwc.dtype == torch.bfloat16 and tuple(eng.lat.shape) == (2, 4, 16, 16) and tuple(eng.canvas.shape) == (1, 4, 16, 24)
    assert eng.geometry is geom and eng.P == 1
    assert torch.isfinite(got).all() and torch.equal(got, fresh)
    after = get_unet_attn_processors(unet)
    assert after.keys() == before.keys() and all(after[k] is before[k] for k in before)


# ------------------------------------------------------------------------------------------------ FFHQ size, bf16
FN = 4


def test_ffhq_bf16_graph_vs_fp32_eager(monkeypatch):
    from afldm_amd.schedulers.schedule import Schedule
    from afldm_amd.utils import randn_tensor
    u32, _, _ = build("ffhq", torch.float32)
    u16, _, _ = build("ffhq", torch.bfloat16)
    p32, p16 = _ldm(u32), _ldm(u16)
    s = u32.config.sample_size
    gen = torch.Generator().manual_seed(21)
    plain = torch.randn(3, 4, s, s, generator=gen)                        # as many planes as the canvas has windows
    x = torch.randn(1, 4, s, 2 * s, generator=gen)
    # the yardstick: the deterministic bf16 DDIM graph run against its fp32 run over as many evaluations
    det = rel_rms(p16(latents=plain, num_inference_steps=FN, output_type="latent").float(),
                  p32(latents=plain, num_inference_steps=FN, output_type="latent", use_graph=False))
    kw = dict(stride=s // 2, eta=0.7, num_inference_steps=FN, latents=x)
    # the fp32 eager loop on the draws of the bf16 run: a bf16 model draws its noise in bf16
    with monkeypatch.context() as mp:
        mp.setattr(Schedule, "draw_noise", lambda self, shape, generator, device, model_dtype:
                   randn_tensor(shape, generator=generator, device=device, dtype=torch.bfloat16))
        want = p32.panorama_latents(s, 2 * s, generator=torch.Generator().manual_seed(41), use_graph=False, **kw)
    got = p16.panorama_latents(s, 2 * s, generator=torch.Generator().manual_seed(41), **kw)
    (eng,) = p16._pano_engines.values()
    assert eng.geometry.nwin == 3 and got.dtype == torch.float32 and tuple(got.shape) == (1, 4, s, 2 * s)
    assert torch.isfinite(got).all()
    err = rel_rms(got, want)
    err_eager = rel_rms(p16.panorama_latents(s, 2 * s, generator=torch.Generator().manual_seed(41), use_graph=False, **kw), want)
    print(f"[FFHQ panorama {s} x {2 * s}, stride {s // 2}, eta=0.7, {FN} evaluations] bf16 rel-RMS vs the fp32 eager loop: graph {err:.3e}, "
          f"bf16 eager loop {err_eager:.3e}; bf16 DDIM graph vs fp32, {FN} steps, batch 3: {det:.3e}")
    assert err <= 1.5 * det, (err, det)


# ------------------------------------------------------------------------------------------------ pixels
def test_tiny_pixel_path_is_the_feathered_blend_of_the_window_decodes(tiny, monkeypatch):
    from afldm_amd.panorama import feather
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from test_gpu_pano import mean_bound
    from test_gpu_vae import build_vae
    vae, _, _ = build_vae(torch.float32)
    pipe = MyLDMPipeline(vae, tiny["unet"], ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    decodes = []
    plain_decode = vae.decode

    def recording(z, *a, **k):
        out = plain_decode(z, *a, **k)
        decodes.append((z.detach().cpu(), out.sample.detach().cpu()))
        return out
    monkeypatch.setattr(vae, "decode", recording)
    kw = dict(height=128, width=192, stride=64, num_inference_steps=2, batch_size=2)
    pt = pipe.panorama(generator=torch.Generator().manual_seed(2), output_type="pt", **kw)
    assert pt.dtype == torch.float32 and tuple(pt.shape) == (2, 3, 128, 192) and torch.isfinite(pt).all()
    canvas = pipe.panorama(generator=torch.Generator().manual_seed(2), output_type="latent", **kw)
    assert tuple(canvas.shape) == (2, 4, 16, 24) and len(decodes) == 2          # one decode of batch nwin per canvas
    g = pipe.panorama_geometry(16, 24, 8)
    # what was decoded: the windows of the sampled canvas, at the sampling origins
    fed = torch.cat([z for z, _ in decodes])
    assert g.nwin == 2                                                    # (the division by scaling_factor is rounded on the device)
    torch.testing.assert_close(fed * vae.config.scaling_factor, po.crop(canvas.cpu(), g), rtol=1e-6, atol=1e-6)
    dec = torch.cat([d for _, d in decodes])
    t = torch.tensor(feather(128))
    wt = torch.outer(t, t)
    want = po.fuse(dec, wt, g.scaled(8))
    tol = 2e-6 * float(want.abs().max()) + 2.0 * mean_bound(dec, wt, g.scaled(8))
    err = float((pt.cpu().double() - want).abs().max())
    print(f"[tiny panorama 128 x 192 pixels] blend max-abs error vs float64 {err:.2e} of {tol:.2e} allowed")
    assert err <= tol
    out = pipe.panorama(generator=torch.Generator().manual_seed(2), **kw)
    assert len(out.images) == 2 and out.images[0].size == (192, 128)
    with pytest.raises(ValueError):
        pipe.panorama(height=128, width=100)
    with pytest.raises(NotImplementedError):
        tiny["pipe"].panorama(height=128, width=192)                       # no VAE
