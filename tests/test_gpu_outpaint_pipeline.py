"""Outpainting end to end on MI355X: MyLDMPipeline.outpaint_latents on replayed graphs (OutpaintEngine) against its own eager loop
(same generator, same draws), against the CPU oracle UNet driven by the float64 restatement of tests/outpaint_oracle.py, against
inpaint_latents where the canvas is one window and against panorama_latents where nothing is kept, under a roll of a circular
canvas, the engine cache, an FFHQ-size bf16 run, and the pixel path.  Graph against eager, the two reductions and the roll:
rel-RMS 1e-5; fp32 against the oracle: 1e-3 (the sibling files' bounds for the same comparisons).  bf16: no number fixed in
advance - the graph run may differ from the fp32 eager loop on the same draws by 1.5x what the deterministic bf16 DDIM graph run
differs from its fp32 run over as many evaluations (test_gpu_pano_pipeline's construction)."""
import pytest
import torch

import outpaint_oracle as oo
from test_gpu_dpm import _run_across_a_dtype_change, build, rel_rms
from test_gpu_sde import _gens, _ldm, _same_state

pytestmark = pytest.mark.gpu

N = 6
JUMP = dict(jump_length=2, jump_n_sample=2)


@pytest.fixture(scope="module")
def tiny():
    unet, cfg, sd = build("tiny", torch.float32)
    return dict(unet=unet, cfg=cfg, sd=sd, pipe=_ldm(unet))


def content(P, Hc, Wc, left, width=16, seed=9, C=4):
    """A known canvas (random where kept, zeros elsewhere) and its hard mask [1, 1, Hc, Wc]: columns left .. left + width - 1, modulo
    Wc."""
    cols = torch.arange(left, left + width) % Wc
    known = torch.zeros(P, C, Hc, Wc)
    known[..., cols] = torch.randn(P, C, Hc, width, generator=torch.Generator().manual_seed(seed))
    mask = torch.zeros(1, 1, Hc, Wc)
    mask[..., cols] = 1.0
    return known, mask


def kept(canvas, known, mask):
    keep = (mask == 1.0).expand_as(known)
    return int(keep.sum()) > 0 and torch.equal(canvas.cpu()[keep], known[keep])


@pytest.mark.parametrize("eta,kind", [(0.0, "cpu"), (0.7, "cpu"), (0.7, "cuda"), (0.7, "list")])
def test_tiny_graph_vs_eager_loop(tiny, eta, kind):
    pipe = tiny["pipe"]
    known, mask = content(2, 16, 40, 12)
    kw = dict(stride=8, eta=eta, num_inference_steps=N, **JUMP)
    ga, gb, gc, gd = _gens(kind, 11), _gens(kind, 11), _gens(kind, 11), _gens(kind, 12)
    a = pipe.outpaint_latents(known, mask, generator=ga, **kw)
    assert a.dtype == torch.float32 and tuple(a.shape) == (2, 4, 16, 40)
    (key,) = pipe._outpaint_engines
    eng = pipe._outpaint_engines[key]
    g, sched = eng.geometry, eng.schedule
    assert (g.oy, g.ox, g.nwin) == ((0,), (0, 8, 16, 24), 4) and sched.kind == "outpaint" and eng.branches == 1
    assert len(sched.rows) > N and any(r[10] != 0.0 for r in sched.rows)                          # some evaluations jump back up
    assert tuple(eng.lat.shape) == (8, 4, 16, 16) and tuple(eng.canvas.shape) == (2, 4, 16, 40)
    assert tuple(eng.noise.shape) == (len(sched.rows), 3, 2, 4, 16, 40) and tuple(eng.mask.shape) == (2, 1, 16, 40)
    b = pipe.outpaint_latents(known, mask, generator=gb, use_graph=False, **kw)
    err = rel_rms(a, b)
    print(f"[tiny outpaint 16 x 40, stride 8, N={N}, {len(sched.rows)} evaluations, eta={eta}, {kind} generator] graph vs eager loop "
          f"rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert kept(a, known, mask) and kept(b, known, mask)                                         # kept latents: exactly the input's
    assert torch.equal(a, pipe.outpaint_latents(known, mask, generator=gc, **kw))                # seeded: bit-identical
    assert pipe._outpaint_engines[key] is eng
    other = pipe.outpaint_latents(known, mask, generator=gd, **kw)                               # another seed: another sample
    assert rel_rms(other, a) > 1e-2 and kept(other, known, mask)


def test_tiny_vs_oracle(tiny):
    """16 x 24 canvas, stride 8, N = 4 (7 evaluations), eta = 0.7: the oracle UNet on the CPU under the float64 loop, drawing the same
    noise from the same CPU generator."""
    from oracle import unet as ou
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = tiny["pipe"]
    known, mask = content(1, 16, 24, 4, width=12)
    x = torch.randn(1, 4, 16, 24, generator=torch.Generator().manual_seed(4))
    kw = dict(stride=8, eta=0.7, num_inference_steps=4, **JUMP)
    got = pipe.outpaint_latents(known, mask, latents=x, generator=torch.Generator().manual_seed(31), **kw)
    g = pipe.panorama_geometry(16, 24, 8)
    assert g.ox == (0, 8)
    gen = torch.Generator().manual_seed(31)
    sched = ffhq_ddim_scheduler().outpaint_schedule(4, 0.7, 2, 2)
    want = oo.sample(lambda w, t: ou.unet_forward(tiny["sd"], tiny["cfg"], w, t), x, known, mask, g, sched,
                     lambda: torch.randn(x.shape, generator=gen))
    err = rel_rms(got, want)
    print(f"[tiny outpaint 16 x 24, {len(sched.rows)} evaluations, eta=0.7] fp32 rel-RMS vs the oracle loop {err:.3e}")
    assert err <= 1e-3, err
    assert kept(got, known, mask)


def test_tiny_single_window_is_inpaint_and_no_mask_is_the_panorama(tiny):
    pipe = tiny["pipe"]
    # a canvas of one window: RePaint on that window, the same draws in the same order
    known, mask = content(2, 16, 16, 3, width=7)
    for eta in (0.0, 0.7):
        kw = dict(num_inference_steps=N, eta=eta, **JUMP)
        a = pipe.outpaint_latents(known, mask, generator=torch.Generator().manual_seed(1), **kw)
        b = pipe.inpaint_latents(known, mask, generator=torch.Generator().manual_seed(1), **kw)
        err = rel_rms(a, b)
        print(f"[tiny outpaint 16 x 16 = one window, eta={eta}] vs inpaint_latents rel-RMS {err:.2e}")
        assert err <= 1e-5, err
    # nothing kept, no jumps, eta = 0: MultiDiffusion from the same start canvas (z_k is drawn, and weighs 0)
    x = torch.randn(2, 4, 16, 40, generator=torch.Generator().manual_seed(3))
    known, _ = content(2, 16, 40, 12)
    a = pipe.outpaint_latents(known, torch.zeros(1, 1, 16, 40), stride=8, num_inference_steps=N, jump_length=2, jump_n_sample=1,
                              latents=x, generator=torch.Generator().manual_seed(1))
    b = pipe.panorama_latents(16, 40, stride=8, num_inference_steps=N, latents=x)
    err = rel_rms(a, b)
    print(f"[tiny outpaint 16 x 40, mask = 0, no jumps, eta=0] vs panorama_latents rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    # shapes
    with pytest.raises(ValueError):
        pipe.outpaint_latents(known, torch.zeros(1, 1, 16, 32))                                 # a mask of another canvas
    with pytest.raises(ValueError):
        pipe.outpaint_latents(known, torch.zeros(3, 1, 16, 40))
    with pytest.raises(ValueError):
        pipe.outpaint_latents(known[:, :, :8], torch.zeros(1, 1, 8, 40))                        # a canvas smaller than the window
    with pytest.raises(ValueError):
        pipe.outpaint_latents(known, torch.zeros(1, 1, 16, 40), latents=x[..., :32])


def test_tiny_circular_canvas_commutes_with_a_roll_by_the_stride(tiny, monkeypatch):
    """The roll has to reach the noise too: the draws are replaced by a fixed list, rolled like the canvas."""
    from afldm_amd.schedulers.schedule import Schedule
    pipe = tiny["pipe"]
    known, mask = content(1, 16, 32, 26)                                   # the kept columns straddle the seam
    assert float(mask[0, 0, 0, 0]) == float(mask[0, 0, 0, 31]) == 1.0
    x = torch.randn(1, 4, 16, 32, generator=torch.Generator().manual_seed(5))
    zs = [torch.randn(1, 4, 16, 32, generator=torch.Generator().manual_seed(50 + i)) for i in range(40)]
    kw = dict(stride=8, circular=True, num_inference_steps=N, eta=0.7, **JUMP)

    def run(shift, **over):
        it = iter(zs)
        with monkeypatch.context() as mp:
            mp.setattr(Schedule, "draw_noise", lambda self, shape, generator, device, model_dtype: next(it).roll(shift, -1))
            return pipe.outpaint_latents(known.roll(shift, -1), mask.roll(shift, -1), latents=x.roll(shift, -1), **dict(kw, **over))
    a = run(0)
    (eng,) = pipe._outpaint_engines.values()
    assert eng.geometry.wrap_x and eng.geometry.ox == (0, 8, 16, 24)
    b = run(8)
    err = rel_rms(b, a.roll(8, -1))
    print(f"[tiny circular outpaint 16 x 32, stride 8, eta=0.7] roll by 8: rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert kept(a, known, mask) and kept(b, known.roll(8, -1), mask.roll(8, -1))
    # the seam is sampled like any other column: not circular, the same inputs give another canvas
    assert rel_rms(run(0, circular=False), a) > 1e-3


def test_tiny_engine_cache(tiny):
    pipe = tiny["pipe"]
    kw = dict(stride=8, num_inference_steps=N, **JUMP)
    k1, m1 = content(1, 16, 40, 12, seed=6)
    k2, m2 = content(1, 16, 40, 20, width=10, seed=7)
    x = torch.randn(1, 4, 16, 40, generator=torch.Generator().manual_seed(8))

    def run(known, mask, **over):
        return pipe.outpaint_latents(known, mask, latents=x[..., :known.shape[-1]], generator=torch.Generator().manual_seed(2),
                                     **dict(kw, **over))
    a = run(k1, m1)
    (key,) = pipe._outpaint_engines
    eng = pipe._outpaint_engines[key]
    graphs = (eng.graph, eng.graph_multi)
    assert graphs[0] is not None and graphs[1] is not None               # the 1-step and the steps_per_graph-step graph
    b = run(k2, m2)                                                      # other content, another mask: the same engine, no recapture
    assert pipe._outpaint_engines[key] is eng and (eng.graph, eng.graph_multi) == graphs
    assert rel_rms(b, a) > 1e-2 and kept(b, k2, m2) and rel_rms(b, run(k2, m2, use_graph=False)) <= 1e-5
    assert torch.equal(run(k1, m1), a)                                   # ... and back
    run(k1[..., :32], m1[..., :32])                                      # another width: another geometry replaces the entry
    (key2,) = pipe._outpaint_engines
    eng2 = pipe._outpaint_engines[key2]
    assert key2 != key and eng2 is not eng and eng2.geometry.Wc == 32
    pipe.outpaint_latents(k1[..., :32], m1[..., :32], generator=torch.Generator().manual_seed(2), **dict(kw, jump_n_sample=3))
    (key3,) = pipe._outpaint_engines
    assert key3 != key2 and pipe._outpaint_engines[key3] is not eng2       # ... and so does another schedule
    from afldm_amd.engine import DenoiseEngine, OutpaintEngine, PanoramaEngine
    sched = pipe.scheduler.outpaint_schedule(N, 0.0, 2, 2)
    g = pipe.panorama_geometry(16, 40, 8)
    with pytest.raises(NotImplementedError):                              # an "outpaint" schedule is OutpaintEngine's alone
        DenoiseEngine(tiny["unet"], sched, 4, len(sched.rows))
    with pytest.raises(NotImplementedError):
        PanoramaEngine(tiny["unet"], sched, 4, len(sched.rows), geometry=g)
    with pytest.raises(NotImplementedError):                              # ... and it takes no other
        OutpaintEngine(tiny["unet"], pipe.scheduler.repaint_schedule(N, 0.0, 2, 2), 4, len(sched.rows), geometry=g)
    # the engine's own checks of known=
    with pytest.raises(ValueError):
        eng.run(x, draw=lambda: x)
    with pytest.raises(ValueError):
        eng.run(x, draw=lambda: x, known=(k1[..., :32], m1))
    with pytest.raises(ValueError):
        eng.run(x, draw=lambda: x, known=(k1, m1[..., :32]))


# ------------------------------------------------------------------------------------------------ a dtype change under a live engine
def test_tiny_engine_survives_a_dtype_change():
    from afldm_amd.engine import OutpaintEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, _, _ = build("tiny", torch.float32)
    geom, sched = _ldm(unet).panorama_geometry(16, 24, 8), ffhq_ddim_scheduler().outpaint_schedule(3, 0.7, 2, 2)
    n = len(sched.rows)
    x = torch.randn(1, 4, 16, 24, generator=torch.Generator().manual_seed(4))
    known, mask = content(1, 16, 24, 4, width=12)

    class Bound(OutpaintEngine):
        def run(self, canvas):
            gen = torch.Generator().manual_seed(17)
            return super().run(canvas, draw=lambda: torch.randn(canvas.shape, generator=gen), known=(known, mask))
    eng, said, got, fresh = _run_across_a_dtype_change(lambda: Bound(unet, sched, geom.nwin, n, geometry=geom), x)
    assert said == [True]
    assert eng.x_nhwc.dtype == torch.bfloat16 and tuple(eng.lat.shape) == (2, 4, 16, 16) and tuple(eng.canvas.shape) == (1, 4, 16, 24)
    assert eng.geometry is geom and eng.P == 1 and tuple(eng.noise.shape) == (n, 3, 1, 4, 16, 24)
    assert torch.isfinite(got).all() and torch.equal(got, fresh) and kept(got, known, mask)
    eng.check_errors()


# ------------------------------------------------------------------------------------------------ FFHQ size, bf16
def test_ffhq_bf16_graph_vs_fp32_eager(monkeypatch):
    from afldm_amd.schedulers.schedule import Schedule
    from afldm_amd.utils import randn_tensor
    u32, _, _ = build("ffhq", torch.float32)
    u16, _, _ = build("ffhq", torch.bfloat16)
    p32, p16 = _ldm(u32), _ldm(u16)
    s = u32.config.sample_size
    kw = dict(stride=s // 2, eta=0.7, num_inference_steps=3, **JUMP)
    evals = len(p32.scheduler.outpaint_schedule(3, 0.7, 2, 2).rows)
    assert evals == 5
    gen = torch.Generator().manual_seed(21)
    plain = torch.randn(3, 4, s, s, generator=gen)                        # as many planes as the canvas has windows
    x = torch.randn(1, 4, s, 2 * s, generator=gen)
    known, mask = content(1, s, 2 * s, s // 2, width=s, seed=22)
    known = known.bfloat16().float()
    # the yardstick: the deterministic bf16 DDIM graph run against its fp32 run over as many evaluations
    det = rel_rms(p16(latents=plain, num_inference_steps=evals, output_type="latent").float(),
                  p32(latents=plain, num_inference_steps=evals, output_type="latent", use_graph=False))
    # the fp32 eager loop on the draws of the bf16 run: a bf16 model draws its noise in bf16
    with monkeypatch.context() as mp:
        mp.setattr(Schedule, "draw_noise", lambda self, shape, generator, device, model_dtype:
                   randn_tensor(shape, generator=generator, device=device, dtype=torch.bfloat16))
        want = p32.outpaint_latents(known, mask, latents=x, generator=torch.Generator().manual_seed(41), use_graph=False, **kw)
    got = p16.outpaint_latents(known, mask, latents=x, generator=torch.Generator().manual_seed(41), **kw)
    (eng,) = p16._outpaint_engines.values()
    assert eng.geometry.nwin == 3 and got.dtype == torch.float32 and tuple(got.shape) == (1, 4, s, 2 * s)
    assert torch.isfinite(got).all()
    err = rel_rms(got, want)
    print(f"[FFHQ outpaint {s} x {2 * s}, stride {s // 2}, eta=0.7, {evals} evaluations] bf16 graph rel-RMS vs the fp32 eager loop "
          f"{err:.3e}; bf16 DDIM graph vs fp32, {evals} steps, batch 3: {det:.3e}")
    assert err <= 1.5 * det, (err, det)
    keep = (mask == 1.0).expand_as(known)
    assert torch.equal(got.cpu()[keep], known.bfloat16().float()[keep])


# ------------------------------------------------------------------------------------------------ pixels
def test_tiny_pixel_path(tiny):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from test_gpu_vae import build_vae
    vae, _, _ = build_vae(torch.float32)
    pipe = MyLDMPipeline(vae, tiny["unet"], ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    image = (torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(2)) * 2 - 1)
    kw = dict(stride=64, num_inference_steps=2, jump_length=1, jump_n_sample=2)

    def run(**over):
        return pipe.outpaint(image, 128, 192, generator=torch.Generator().manual_seed(3), **dict(kw, **over))
    pt = run(output_type="pt")
    assert pt.dtype == torch.float32 and tuple(pt.shape) == (2, 3, 128, 192) and torch.isfinite(pt).all()
    raw = run(output_type="pt", composite=False)
    img = image.cuda()
    assert torch.equal(pt[..., 32:160], img)                              # centred: the input's pixels, exactly
    assert not torch.equal(raw[..., 32:160], img)
    assert torch.equal(pt[..., :32], raw[..., :32]) and torch.equal(pt[..., 160:], raw[..., 160:])
    canvas = run(output_type="latent")
    assert canvas.dtype == torch.float32 and tuple(canvas.shape) == (2, 4, 16, 24)
    z = pipe._encode_mode(img).float()
    assert torch.equal(canvas[..., 4:20], z)                              # the kept latents are the encode's
    # a margin of one latent: the kept rectangle loses 8 pixels per side
    pm = run(output_type="pt", keep_margin=1)
    rm = run(output_type="pt", keep_margin=1, composite=False)
    assert torch.equal(pm[:, :, 8:120, 40:152], img[:, :, 8:120, 8:120]) and not torch.equal(rm[:, :, 8:120, 40:152], img[:, :, 8:120, 8:120])
    outside = torch.ones(128, 192, dtype=torch.bool, device="cuda")
    outside[8:120, 40:152] = False
    assert torch.equal(pm[:, :, outside], rm[:, :, outside])
    cm = run(output_type="latent", keep_margin=1)
    assert torch.equal(cm[:, :, 1:15, 5:19], z[:, :, 1:15, 1:15]) and not torch.equal(cm[..., 4:20], z)
    # placement: flush left; wrapped on a circular canvas
    left = run(output_type="pt", left=0)
    assert torch.equal(left[..., :128], img)
    wrapped = run(output_type="pt", left=128, circular=True)
    assert torch.equal(wrapped[..., 128:], img[..., :64]) and torch.equal(wrapped[..., :64], img[..., 64:])
    out = run()
    assert len(out.images) == 2 and out.images[0].size == (192, 128)
    for bad in (dict(width=100), dict(left=4), dict(left=72), dict(top=8), dict(keep_margin=8)):
        with pytest.raises(ValueError):
            pipe.outpaint(image, **dict(dict(height=128, width=192), **bad))
    with pytest.raises(ValueError):
        pipe.outpaint(image[..., :64], 128, 192)
    with pytest.raises(NotImplementedError):
        tiny["pipe"].outpaint(image, 128, 192)                            # no VAE
