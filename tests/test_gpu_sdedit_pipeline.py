"""Image-to-image sampling (SDEdit with a change map) on MI355X, tiny UNet and VAE: MyLDMPipeline.img2img_latents on replayed
graphs against its own eager loop (same generator, same draws), against the plain sampler over the same truncated timesteps,
against the CPU oracle UNet under the float64 loop of tests/sdedit_oracle.py, the invariants of the change map, the engine cache,
bf16, and img2img end to end.  N = 8, strength = 0.5: n = 4 evaluations.

Bounds.  Graph against eager and against the plain sampler: rel-RMS 1e-5; fp32 against the oracle: 1e-3 (tests/test_gpu_repaint.py's
bounds for the same comparisons).  bf16: no number fixed in advance - the bf16 run may differ from the fp32 run on the same inputs
by 1.5x (RePaint's factor) what the plain bf16 sampler, its result delivered in bf16 as the pipeline delivers it, differs from the
plain fp32 one over the same four timesteps from the same start, measured in the same test."""
import pytest
import torch
import torch.nn.functional as F

import sdedit_oracle as so
from test_gpu_dpm import build, rel_rms
from test_gpu_sde import _gens, _ldm, _same_state

pytestmark = pytest.mark.gpu

N, STRENGTH, EVALS = 8, 0.5, 4
LEVELS = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])


def level_map(shape, seed):
    m = LEVELS[torch.randint(0, 5, shape, generator=torch.Generator().manual_seed(seed))]
    m.reshape(-1)[:5] = LEVELS
    return m


@pytest.fixture(scope="module")
def tiny():
    unet, cfg, sd = build("tiny", torch.float32)
    g = torch.Generator().manual_seed(3)
    orig = 0.8 * torch.randn(2, 4, 16, 16, generator=g)
    z = torch.randn(2, 4, 16, 16, generator=g)
    return dict(unet=unet, cfg=cfg, sd=sd, pipe=_ldm(unet), orig=orig, z=z, cmap=level_map((2, 1, 16, 16), 4),
                one=level_map((1, 1, 16, 16), 5))


def plain_sampler(unet, x_start):
    """The plain eta = 0 sampler over the last EVALS of the N timesteps, on the engine every other sampler uses."""
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.schedulers.schedule import Schedule
    s = ffhq_ddim_scheduler()
    s.set_timesteps(N)
    ts = s._timesteps_host[N - EVALS:]
    sched = Schedule.of(s, "ddim", ts, s.coefficients, _test_truncated=(N, EVALS))
    return DenoiseEngine(unet, sched, x_start.shape[0], EVALS).run(x_start)


def start_of(orig, z):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    return so.x_start(orig, z, ffhq_ddim_scheduler().sdedit_start(N, STRENGTH))


# ------------------------------------------------------------------------------------------------ graph against eager
@pytest.mark.parametrize("eta,kind", [(eta, kind) for eta in (0.0, 0.7) for kind in ("cpu", "cuda", "list")])
def test_graph_vs_eager_loop(tiny, eta, kind):
    pipe, orig, cmap = tiny["pipe"], tiny["orig"], tiny["cmap"]
    kw = dict(strength=STRENGTH, change_map=cmap, num_inference_steps=N, eta=eta)
    ga, gb, gc = _gens(kind, 11), _gens(kind, 11), _gens(kind, 11)
    a = pipe.img2img_latents(orig, generator=ga, **kw)
    (key,) = pipe._sdedit_engines
    eng = pipe._sdedit_engines[key]
    assert type(eng).__name__ == "SDEditEngine" and eng.schedule.kind == "sdedit" and len(eng.schedule.timesteps) == EVALS
    assert (eng.noise is None) == (eta == 0.0) and (eta == 0.0 or tuple(eng.noise.shape) == (EVALS, 2, 4, 16, 16))
    assert "_engines" not in pipe.__dict__ or key not in pipe._engines
    b = pipe.img2img_latents(orig, generator=gb, use_graph=False, **kw)
    err = rel_rms(a, b)
    print(f"[tiny img2img N={N} strength={STRENGTH} eta={eta}, {EVALS} evaluations, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)                                           # the same draws: z, then z_u per evaluation that draws
    assert torch.equal(a, pipe.img2img_latents(orig, generator=gc, **kw)) and pipe._sdedit_engines[key] is eng
    assert a.dtype == torch.float32 and tuple(a.shape) == (2, 4, 16, 16)
    keep = (cmap == 0).expand_as(orig)
    assert torch.equal(a.cpu()[keep], orig[keep]) and torch.equal(b.cpu()[keep], orig[keep])


def test_steps_per_graph_one_and_two_are_bit_identical(tiny, monkeypatch):
    outs = []
    for spg in ("1", "2"):
        monkeypatch.setenv("AFLDM_STEPS_PER_GRAPH", spg)
        pipe = _ldm(tiny["unet"])                                        # a pipeline of its own: the engine is made under the setting
        outs.append(pipe.img2img_latents(tiny["orig"], STRENGTH, tiny["cmap"], N, eta=0.7, generator=torch.Generator().manual_seed(6)))
        (eng,) = pipe._sdedit_engines.values()
        assert eng.steps_per_graph == int(spg) and eng.graph is not None and (eng.graph_multi is not None) == (spg == "2")
    assert torch.equal(outs[0], outs[1])


def test_two_parallel_branches(tiny, monkeypatch):
    """AFLDM_BRANCHES=2: every branch takes its batch slice of the original, the map, the fixed noise and the step's noise."""
    from afldm_amd import trunk
    monkeypatch.setattr(trunk, "_BLOCKED", set(trunk._BLOCKED))
    monkeypatch.setenv("AFLDM_BRANCHES", "2")
    pipe = _ldm(tiny["unet"])                                            # a pipeline of its own: the engine is made under the setting
    kw = dict(strength=STRENGTH, change_map=tiny["cmap"], num_inference_steps=N, eta=0.7)
    got = pipe.img2img_latents(tiny["orig"], generator=torch.Generator().manual_seed(6), **kw)
    (eng,) = pipe._sdedit_engines.values()
    assert eng.branches == 2
    want = pipe.img2img_latents(tiny["orig"], generator=torch.Generator().manual_seed(6), use_graph=False, **kw)
    err = rel_rms(got, want)
    print(f"[tiny img2img, two branches, eta=0.7] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err


# ------------------------------------------------------------------------------------------------ invariants
def test_no_map_is_the_plain_sampler_over_the_truncated_timesteps(tiny):
    pipe, orig, z = tiny["pipe"], tiny["orig"], tiny["z"]
    got = pipe.img2img_latents(orig, STRENGTH, None, N, noise=z)
    want = plain_sampler(tiny["unet"], start_of(orig, z).float())
    err = rel_rms(got, want)
    print(f"[tiny img2img, no change map] vs the plain sampler over the last {EVALS} of {N} timesteps from the same start: rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    ones = pipe.img2img_latents(orig, STRENGTH, torch.ones(1, 1, 16, 16), N, noise=z)
    assert torch.equal(ones, got)                                        # None means all ones
    # the draw: without noise= the run's z comes from the generator, in the model's dtype
    g = torch.Generator().manual_seed(2)
    drawn = pipe.img2img_latents(orig, STRENGTH, None, N, generator=g)
    zz = torch.randn(orig.shape, generator=torch.Generator().manual_seed(2))
    assert torch.equal(drawn, pipe.img2img_latents(orig, STRENGTH, None, N, noise=zz))


def test_kept_region_is_exact_and_the_rest_changes(tiny):
    pipe, orig, z = tiny["pipe"], tiny["orig"], tiny["z"]
    cmap = torch.ones(1, 1, 16, 16)
    cmap[..., :8] = 0.0
    for use_graph in (True, False):
        out = pipe.img2img_latents(orig, STRENGTH, cmap, N, noise=z, use_graph=use_graph).cpu()
        assert torch.equal(out[..., :8], orig[..., :8]), use_graph
        err = rel_rms(out[..., 8:], orig[..., 8:])
        print(f"[tiny img2img, left half kept, use_graph={use_graph}] the right half differs from the original by rel-RMS {err:.2e}")
        assert err > 1e-2
    # everything kept: the original comes back whatever is drawn
    out = pipe.img2img_latents(orig, STRENGTH, torch.zeros(1, 1, 16, 16), N, eta=0.7, generator=torch.Generator().manual_seed(1))
    assert torch.equal(out.cpu(), orig)


def test_cached_engine_reads_the_fixed_buffers(tiny):
    """A second run on the cached engine - another image, another map, another noise - is a fresh engine's result, bit for bit:
    the graphs hold the buffers' addresses only."""
    unet, orig, z, cmap = tiny["unet"], tiny["orig"], tiny["z"], tiny["cmap"]
    g = torch.Generator().manual_seed(17)
    orig2, z2 = torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 4, 16, 16, generator=g)
    used = _ldm(unet)
    first = used.img2img_latents(orig, STRENGTH, cmap, N, noise=z)
    (eng,) = used._sdedit_engines.values()
    graphs = (eng.graph, eng.graph_multi)
    second = used.img2img_latents(orig2, STRENGTH, tiny["one"], N, noise=z2)          # (a batch-1 map this time)
    (again,) = used._sdedit_engines.values()
    assert again is eng and (eng.graph, eng.graph_multi) == graphs and graphs[0] is not None
    fresh = _ldm(unet).img2img_latents(orig2, STRENGTH, tiny["one"], N, noise=z2)
    assert torch.equal(second, fresh) and rel_rms(second, first) > 1e-2
    with pytest.raises(ValueError):
        eng.run(orig, draw=None)                                         # no known=(orig, cmap, z)
    with pytest.raises(ValueError):
        eng.run(orig, known=(orig, cmap[:, :, :8], z))
    with pytest.raises(ValueError):
        eng.run(orig, known=(orig, cmap, z[:1]))


# ------------------------------------------------------------------------------------------------ oracle
def test_vs_oracle_loop(tiny):
    """The oracle UNet on the CPU under the float64 loop, the same z and map."""
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from oracle import unet as ou
    pipe, orig, z, cmap = tiny["pipe"], tiny["orig"], tiny["z"], tiny["cmap"]
    got = pipe.img2img_latents(orig, STRENGTH, cmap, N, noise=z)
    s = ffhq_ddim_scheduler()
    sched = s.sdedit_schedule(N, STRENGTH)
    want = so.sample(lambda x, t: ou.unet_forward(tiny["sd"], tiny["cfg"], x.float(), t).double(), orig, cmap, z, sched,
                     s.sdedit_start(N, STRENGTH))
    err = rel_rms(got, want)
    print(f"[tiny img2img N={N} strength={STRENGTH} eta=0, {EVALS} evaluations] fp32 rel-RMS vs the oracle loop {err:.3e}")
    assert err <= 1e-3, err
    keep = (cmap == 0).expand_as(orig)
    assert torch.equal(got.cpu()[keep].double(), want[keep])


# ------------------------------------------------------------------------------------------------ bf16
def test_bf16_vs_fp32(tiny):
    orig, z, cmap = tiny["orig"], tiny["z"], tiny["cmap"]
    u16, _, _ = build("tiny", torch.bfloat16)
    p16 = _ldm(u16)
    want = tiny["pipe"].img2img_latents(orig, STRENGTH, cmap, N, noise=z)
    got = p16.img2img_latents(orig, STRENGTH, cmap, N, noise=z)
    assert got.dtype == torch.bfloat16
    start = start_of(orig, z).float()
    # the yardstick delivers what the pipeline delivers: latents in the UNet's dtype.  (The engine returns fp32; compared
    # unrounded, the plain bf16 sampler is 2.74e-4 from the fp32 one, and the 1.66e-3 of the run under test is the rounding of the
    # returned latents to bf16 - relative RMS 2^-8 / sqrt(3) times the mean over a binade, 1.6e-3 - which has to be on both sides.)
    plain16, plain32 = plain_sampler(u16, start), plain_sampler(tiny["unet"], start)
    det = rel_rms(plain16.to(torch.bfloat16).float(), plain32)
    err = rel_rms(got.float(), want)
    eager = rel_rms(p16.img2img_latents(orig, STRENGTH, cmap, N, noise=z, use_graph=False).float(), want)
    print(f"[tiny img2img N={N} strength={STRENGTH}, {EVALS} evaluations, batch 2] bf16 rel-RMS vs the fp32 run: graph {err:.3e}, bf16 eager "
          f"loop {eager:.3e}; plain bf16 sampler vs fp32 over the same timesteps: {det:.3e} as delivered, "
          f"{rel_rms(plain16, plain32):.3e} before the rounding to bf16")
    assert err <= 1.5 * det, (err, det)
    keep = (cmap == 0).expand_as(orig)
    assert torch.equal(got.float().cpu()[keep], orig.bfloat16().float()[keep])


# ------------------------------------------------------------------------------------------------ end to end
def test_img2img_end_to_end(tiny):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd import harness, ops
    from test_gpu_vae import build_vae
    vae, _, _ = build_vae(torch.float32)
    pipe = MyLDMPipeline(vae, tiny["unet"], ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    s = 16
    r = pipe._vae_ratio()
    S = s * r
    g = torch.Generator().manual_seed(9)
    image = F.interpolate(torch.rand(2, 3, 8, 8, generator=g) * 2 - 1, size=(S, S), mode="bicubic", align_corners=False).clamp(-1, 1)
    cmap = torch.ones(1, 1, S, S)
    cmap[..., : S // 2 + 3] = 0.0                                        # (an edge that is not on the latent grid)
    cmap[..., S // 2 + 3: 3 * S // 4] = 0.5
    z = torch.randn(2, 4, s, s, generator=g)
    kw = dict(strength=STRENGTH, change_map=cmap, num_inference_steps=N, noise=z)
    pt = pipe.img2img(image, output_type="pt", **kw)
    assert tuple(pt.shape) == (2, 3, S, S) and pt.dtype == torch.float32 and torch.isfinite(pt).all()
    keep = (cmap == 0).expand_as(image)
    assert torch.equal(pt.cpu()[keep], image[keep])                       # composite: kept pixels are the input's, exactly
    raw = pipe.img2img(image, output_type="pt", composite=False, **kw)
    assert not torch.equal(raw.cpu()[keep], image[keep])
    assert torch.equal(raw.float().cpu()[~keep], pt.cpu()[~keep])         # nothing is blended elsewhere: the same sample
    # 'latent' is img2img_latents on the encoded image and the pooled (mean) map
    lat = pipe.img2img(image, output_type="latent", **kw)
    z0 = harness.vae_encode_mode(vae, image.cuda())
    lm = ops.mask_pool(cmap.cuda(), r, ops.MASK_MEAN)
    assert torch.equal(lm.cpu(), F.avg_pool2d(cmap, r)) and 0.0 < float(lm[0, 0, 0, s // 2]) < 0.5       # the straddling column is soft
    assert torch.equal(lat, pipe.img2img_latents(z0, STRENGTH, lm, N, noise=z))
    kept = (lm.cpu() == 0).expand_as(lat)
    assert torch.equal(lat.cpu()[kept], z0.float().cpu()[kept]) and int(kept.sum()) == 2 * 4 * s * (s // 2)
    # no map: plain SDEdit, nothing composited
    free = pipe.img2img(image, STRENGTH, None, N, noise=z, output_type="pt")
    assert tuple(free.shape) == (2, 3, S, S) and not torch.equal(free.cpu()[keep], image[keep])
    (arr,) = pipe.img2img(image, output_type="np", return_dict=False, **kw)
    assert arr.shape == (2, S, S, 3) and arr.min() >= 0.0 and arr.max() <= 1.0
    out = pipe.img2img(image, **kw)
    assert len(out.images) == 2 and out.images[0].size == (S, S)
