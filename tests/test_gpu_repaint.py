"""RePaint inpainting on the graph-replayed engine (MI355X): afldm_repaint_step / afldm_repaint_step_flat against a float64 torch
restatement, afldm_mask_pool against torch's pooling, MyLDMPipeline.inpaint_latents on replayed graphs against its own eager loop
(same generator, same draws) and against the CPU oracle UNet driven by a float64 loop, the invariants of a RePaint sampler
(all-ones / all-zeros / half masks), and FFHQ-size bf16 runs.

Bounds.  Kernel: rtol 2e-6, atol 2e-6 max|want| - test_sde_step_kernel's, the update being the same length of fp32 chain plus two
multiply-adds.  Graph against eager: rel-RMS 1e-5, fp32 against the oracle: 1e-3 (tests/test_gpu_sde.py's bounds for the same
comparisons, over runs of comparable length).  bf16: no number fixed in advance - the graph run may differ from the fp32 eager loop
on the same inputs by 1.5x what the deterministic bf16 DDIM graph run differs from its fp32 run over as many evaluations."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_dpm import build, rel_rms
from test_gpu_sde import _gens, _ldm, _same_state

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
INF = math.inf
# (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0)
ROWS = [
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.3, 0.8, 0.6, 1.0, 0.0, 0.0),      # no clip, c != 0, no jump
    (1.0, -0.9, -1.0, 1.0, 0.9, 0.4, 0.0, 0.9, 0.43, 0.95, 0.31, 0.0),              # clip, c = 0, jump back up
    (1.0, 0.0, -0.5, 0.5, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0),                  # no slot at all: m known + (1 - m) clamp(x)
    (1.2, -0.5, -2.0, 2.0, 0.6, 0.3, 0.2, 1.0, 0.0, 0.8, 0.6, 0.0),                 # clip, c != 0, jump, the kept part not noised
]
SLOT_COEF = (8, 6, 10)          # the row entries k1, c, u1 that switch the slots z_k, z_u, z_b


def f32(row):
    return [float(v) for v in torch.tensor(row, dtype=torch.float64).to(torch.float32)]


def torch_repaint(x, e, known, m, zs, row):
    """The update in float64 on the fp32-rounded row; zs[j] is not looked at where its coefficient is 0."""
    p, q, lo, hi, a, b, c, k0, k1, u0, u1 = f32(row)[:11]
    x, e, known, m = x.double(), e.double(), known.double(), m.double()
    zk, zu, zb = [z.double() if co != 0.0 else torch.zeros_like(x) for z, co in zip(zs, (k1, c, u1))]
    unknown = a * torch.clamp(p * x + q * e, lo, hi) + b * e + c * zu
    return u0 * (m * (k0 * known + k1 * zk) + (1 - m) * unknown) + u1 * zb


def kernel_inputs(dtype, shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(29)
    x = torch.randn(shape, generator=g)
    x[0, 0, 0, :4] = torch.tensor([0.5, -0.5, 0.75, -3.0])              # on and beyond the bounds of row 2
    x[1, 2, 1, 3] = math.nan
    e = torch.randn(shape, generator=g).to(dtype).float()                # what the kernel reads
    known = torch.randn(shape, generator=g)
    m = (torch.rand(B, 1, H, W, generator=g) < 0.5).float()              # hard, per sample ...
    m[:, :, 1, :] = 0.25                                                 # ... and a soft row
    m[0, 0, 0, :4] = 0.0                                                 # (the clamp probes are generated pixels)
    big = torch.randn(len(ROWS), 3, 2 * B, C, H, W, generator=g)
    return x, e, known, m, big


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, [(3, 4, 16, 16), (2, 3, 5, 5)])))     # 16-byte groups / scalar
def test_repaint_step_kernel(dtype, shape):
    from afldm_amd import ops
    B = shape[0]
    x, e, known, m, big = kernel_inputs(dtype, shape)
    e_nhwc = e.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)
    # NaN in every slot whose coefficient is 0: the kernel must not load it (0 * NaN is not 0)
    poisoned = big.clone()
    for s, row in enumerate(ROWS):
        for j, k in enumerate(SLOT_COEF):
            if row[k] == 0.0:
                poisoned[s, j] = math.nan
    noise = poisoned.cuda()[:, :, B:]                                    # a batch slice of a larger buffer, as a branch passes it
    assert not noise.is_contiguous() and noise.stride(1) == 2 * x.numel()
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    kg, mg = known.cuda(), m.cuda()
    for s, row in enumerate(ROWS):
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        xg = x.cuda()
        out = ops.repaint_step(xg, e_nhwc, kg, mg, noise, coef, idx, advance=False, out=xg)          # x_out aliases x
        assert out.data_ptr() == xg.data_ptr() and int(idx.item()) == s
        want = torch_repaint(x, e, known, m, big[s, :, B:], row)
        got = out.cpu()
        assert torch.isnan(got[1, 2, 1, 3]) and torch.isnan(got).sum() == 1, s                       # x's NaN, and only that one
        torch.testing.assert_close(got.double(), want, rtol=2e-6, atol=2e-6 * float(want.nan_to_num().abs().max()), equal_nan=True)
        if s == 2:
            assert got[0, 0, 0, :4].tolist() == [0.5, -0.5, 0.5, -0.5]
            keep = (m == 1).expand_as(x)
            assert torch.equal(got[keep], known[keep])                                               # kept latents: exact
        # not aliased: x is left alone
        xg = x.cuda()
        out2 = ops.repaint_step(xg, e_nhwc, kg, mg, noise, coef, idx)
        assert out2.data_ptr() != xg.data_ptr() and torch.equal(out2.cpu().nan_to_num(7.0), got.nan_to_num(7.0))
        assert torch.equal(xg.cpu().nan_to_num(7.0), x.nan_to_num(7.0))
    # advance: the kernel reads row 0, then the counter moves on; a second launch reads row 1
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    ops.repaint_step(xg, e_nhwc, kg, mg, noise, coef, idx, advance=True, out=xg)
    ops.repaint_step(xg, e_nhwc, kg, mg, noise, coef, idx, advance=True, out=xg)
    assert int(idx.item()) == 2
    want = torch_repaint(torch_repaint(x, e, known, m, big[0, :, B:], ROWS[0]), e, known, m, big[1, :, B:], ROWS[1])
    # two chained updates: the first one's 2e-6 passes through |u0 (1 - m) a p| < 1 of row 1 and the second adds its own
    torch.testing.assert_close(xg.cpu().double(), want, rtol=1e-5, atol=1e-5 * float(want.nan_to_num().abs().max()), equal_nan=True)


@pytest.mark.parametrize("shape", [(3, 4, 16, 16), (2, 3, 5, 5)])          # 16-byte groups / groups and a scalar tail (150 = 4 * 37 + 2)
def test_repaint_step_flat_kernel(shape):
    from afldm_amd import ops
    B = shape[0]
    x, e, known, m, big = kernel_inputs(torch.float32, shape)
    mfull = m.expand_as(x).contiguous()
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    for s, row in enumerate(ROWS):
        zs = [big[s, j, B:].contiguous().cuda() if row[k] != 0.0 else None for j, k in enumerate(SLOT_COEF)]
        xg = x.cuda()
        out = ops.repaint_step_flat(xg, e.cuda(), known.cuda(), mfull.cuda(), zs, row, out=xg)
        assert out.data_ptr() == xg.data_ptr()
        got = out.cpu()
        want = torch_repaint(x, e, known, m, big[s, :, B:], row)
        assert torch.isnan(got).sum() == 1
        bound = dict(rtol=2e-6, atol=2e-6 * float(want.nan_to_num().abs().max()), equal_nan=True)
        torch.testing.assert_close(got.double(), want, **bound)
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        table = ops.repaint_step(x.cuda(), e.permute(0, 2, 3, 1).contiguous().cuda(), known.cuda(), m.cuda(),
                                 big.cuda()[:, :, B:], coef, idx)
        torch.testing.assert_close(got, table.cpu(), **bound)
        # a slot the row does not use may hold anything
        nan = torch.full_like(x, math.nan).cuda()
        out = ops.repaint_step_flat(x.cuda(), e.cuda(), known.cuda(), mfull.cuda(), [z if z is not None else nan for z in zs], row)
        assert torch.equal(out.cpu().nan_to_num(7.0), got.nan_to_num(7.0))
    with pytest.raises(ValueError):
        ops.repaint_step_flat(x.cuda(), e.cuda(), known.cuda(), mfull.cuda(), [None, None, None], ROWS[0])


@pytest.mark.parametrize("shape,r", [((2, 1, 16, 24), 8), ((1, 1, 9, 6), 3), ((2, 1, 16, 24), 1), ((2, 1, 6, 10), 2)])
def test_mask_pool(shape, r):
    from afldm_amd import ops
    g = torch.Generator().manual_seed(sum(shape) + r)
    hard = (torch.rand(shape, generator=g) < 0.8).float()
    soft = torch.rand(shape, generator=g)
    dyadic = torch.randint(0, 5, shape, generator=g).float() / 4                     # sums exact in fp32: any order gives the same
    for m in (hard, soft, dyadic):
        got = ops.mask_pool(m.cuda(), r).cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], 1, shape[2] // r, shape[3] // r)
        assert torch.equal(got, -F.max_pool2d(-m, r))
        assert torch.equal(ops.mask_pool(m.cuda(), r, ops.MASK_MIN).cpu(), got)
        mean = ops.mask_pool(m.cuda(), r, ops.MASK_MEAN).cpu()
        # avg_pool2d of the fp64 mask, rounded once: fp32 avg_pool2d itself carries the rounding of r * r - 1 fp32 additions
        want = F.avg_pool2d(m.double(), r).float()
        ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -23
        assert ((mean - want).abs() <= ulp).all()
        if r == 1:
            assert torch.equal(got, m) and torch.equal(mean, m)
    assert ((ops.mask_pool(dyadic.cuda(), r, ops.MASK_MEAN).cpu() - F.avg_pool2d(dyadic, r)).abs()
            <= 2.0 ** -23 * F.avg_pool2d(dyadic, r)).all()                             # fp32 avg_pool2d where its sums are exact
    for bad in (5, 0, -1):
        with pytest.raises(ValueError):
            ops.mask_pool(hard.cuda(), bad)


# ------------------------------------------------------------------------------------------------ tiny UNet
N = 6


@pytest.fixture(scope="module")
def tiny():
    unet, cfg, sd = build("tiny", torch.float32)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 16, 16, generator=g)
    known = 0.8 * torch.randn(2, 4, 16, 16, generator=g)
    half = torch.zeros(1, 1, 16, 16)
    half[..., :8] = 1.0
    return dict(unet=unet, cfg=cfg, sd=sd, pipe=_ldm(unet), x=x, known=known, half=half)


@pytest.mark.parametrize("jl,js,eta,kind", [(jl, js, eta, kind) for (jl, js) in [(2, 2), (3, 2)] for eta in (0.0, 0.7)
                                            for kind in ("cpu", "cuda", "list")])
def test_tiny_graph_vs_eager_loop(tiny, jl, js, eta, kind):
    pipe, x, known, half = tiny["pipe"], tiny["x"], tiny["known"], tiny["half"]
    kw = dict(num_inference_steps=N, eta=eta, jump_length=jl, jump_n_sample=js, latents=x)
    ga, gb, gc = _gens(kind, 11), _gens(kind, 11), _gens(kind, 11)
    a = pipe.inpaint_latents(known, half, generator=ga, **kw)
    (key,) = pipe._repaint_engines
    eng = pipe._repaint_engines[key]
    evals = len(eng.schedule.timesteps)
    assert eng.schedule.kind == "repaint" and tuple(eng.noise.shape) == (evals, 3, 2, 4, 16, 16) and evals in (9, 10)
    assert "_engines" not in pipe.__dict__ or key not in pipe._engines
    b = pipe.inpaint_latents(known, half, generator=gb, use_graph=False, **kw)
    err = rel_rms(a, b)
    print(f"[tiny RePaint N={N} J={jl} r={js} eta={eta}, {evals} evaluations, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe.inpaint_latents(known, half, generator=gc, **kw))                     # seeded: bit-identical
    assert pipe._repaint_engines[key] is eng
    # another image and another (per-sample, partly soft) mask: the same engine and graphs, and still the eager loop's result
    graphs = (eng.graph, eng.graph_multi)
    g2 = torch.Generator().manual_seed(5)
    known2 = torch.randn(2, 4, 16, 16, generator=g2)
    mask2 = (torch.rand(2, 1, 16, 16, generator=g2) < 0.5).float()
    mask2[1, 0, 3] = 0.25
    ga, gb = _gens(kind, 12), _gens(kind, 12)
    a2 = pipe.inpaint_latents(known2, mask2, generator=ga, **kw)
    assert pipe._repaint_engines[key] is eng and (eng.graph, eng.graph_multi) == graphs and graphs[0] is not None
    err2 = rel_rms(a2, pipe.inpaint_latents(known2, mask2, generator=gb, use_graph=False, **kw))
    print(f"    second image and mask on the cached engine: rel-RMS {err2:.2e}")
    assert err2 <= 1e-5 and rel_rms(a2, a) > 1e-2
    keep = (mask2 == 1).expand_as(known2)
    assert torch.equal(a2.cpu()[keep], known2[keep])


def test_tiny_invariants(tiny):
    pipe, x, known, half = tiny["pipe"], tiny["x"], tiny["known"], tiny["half"]
    kw = dict(num_inference_steps=N, jump_length=2, jump_n_sample=2, latents=x)
    # everything kept: the known latents come back bit for bit, whatever is drawn
    for use_graph in (True, False):
        out = pipe.inpaint_latents(known, torch.ones(1, 1, 16, 16), eta=0.7, generator=torch.Generator().manual_seed(1),
                                   use_graph=use_graph, **kw)
        assert torch.equal(out.cpu(), known), use_graph
    # nothing kept, eta = 0, no resampling: plain DDIM from the same start
    free = pipe.inpaint_latents(known, torch.zeros(1, 1, 16, 16), num_inference_steps=N, jump_length=2, jump_n_sample=1, latents=x,
                                generator=torch.Generator().manual_seed(1))
    ddim = pipe(latents=x, num_inference_steps=N, output_type="latent")
    err = rel_rms(free, ddim)
    print(f"[tiny RePaint, mask of zeros, eta=0, jump_n_sample=1] vs DDIM {N} steps rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    # half kept: that half is exact, the other half follows the seed and feels the kept half
    a = pipe.inpaint_latents(known, half, eta=0.0, generator=torch.Generator().manual_seed(1), **kw).cpu()
    b = pipe.inpaint_latents(known, half, eta=0.0, generator=torch.Generator().manual_seed(2), **kw).cpu()
    zero = pipe.inpaint_latents(known, torch.zeros(1, 1, 16, 16), eta=0.0, generator=torch.Generator().manual_seed(1), **kw).cpu()
    assert torch.equal(a[..., :8], known[..., :8]) and torch.equal(b[..., :8], known[..., :8])
    # (against the all-zeros mask the draws are the same: the difference is what the UNet makes of the kept half - no size is
    # asked of it, only more than the 1e-5 two runs of the same sampler may differ by)
    assert rel_rms(a[..., 8:], b[..., 8:]) > 1e-2 and rel_rms(a[..., 8:], zero[..., 8:]) > 1e-5
    print(f"[tiny RePaint, half mask] generated half: seed 1 vs 2 rel-RMS {rel_rms(a[..., 8:], b[..., 8:]):.2e}, "
          f"vs the all-zeros mask {rel_rms(a[..., 8:], zero[..., 8:]):.2e}")
    with pytest.raises(ValueError):
        pipe._repaint_engines[next(iter(pipe._repaint_engines))].run(x, draw=lambda: x)              # no known=(z0, mask)


def test_tiny_vs_oracle(tiny):
    """(N, J, r) = (6, 2, 2), eta = 0: the oracle UNet on the CPU under a float64 loop over the schedule's rows, drawing the same
    noise (z_k, then z_b where the row jumps) from the same CPU generator."""
    from oracle import unet as ou
    pipe, x, known, half = tiny["pipe"], tiny["x"], tiny["known"], tiny["half"]
    got = pipe.inpaint_latents(known, half, num_inference_steps=N, eta=0.0, jump_length=2, jump_n_sample=2, latents=x,
                               generator=torch.Generator().manual_seed(31))
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    rp = ffhq_ddim_scheduler().repaint_schedule(N, 0.0, 2, 2)
    gen = torch.Generator().manual_seed(31)
    lat, m, kn = x.double(), half.double(), known.double()
    for t, row in zip(rp.timesteps, rp.rows):
        p, q, lo, hi, a, b, c, k0, k1, u0, u1, _ = row
        eps = ou.unet_forward(tiny["sd"], tiny["cfg"], lat.float(), t).double()
        zk = torch.randn(x.shape, generator=gen).double() if k1 != 0.0 else 0.0
        assert c == 0.0
        zb = torch.randn(x.shape, generator=gen).double() if u1 != 0.0 else 0.0
        unknown = a * torch.clamp(p * lat + q * eps, lo, hi) + b * eps
        lat = u0 * (m * (k0 * kn + k1 * zk) + (1 - m) * unknown) + u1 * zb
    err = rel_rms(got, lat)
    print(f"[tiny RePaint (6, 2, 2) eta=0, 10 evaluations] fp32 rel-RMS vs the oracle loop {err:.3e}")
    assert err <= 1e-3, err


# ------------------------------------------------------------------------------------------------ FFHQ size, bf16
FN, FJ, FR = 4, 2, 2            # 6 evaluations


@pytest.fixture(scope="module")
def ffhq():
    u32, _, _ = build("ffhq", torch.float32)
    u16, _, _ = build("ffhq", torch.bfloat16)
    s = u32.config.sample_size
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 4, s, s, generator=g)
    known = 0.8 * torch.randn(2, 4, s, s, generator=g)
    half = torch.zeros(1, 1, s, s)
    half[..., : s // 2] = 1.0
    p32, p16 = _ldm(u32), _ldm(u16)
    evals = len(p32.scheduler.repaint_schedule(FN, 0.7, FJ, FR).timesteps)
    assert evals == 6
    # the yardstick: the deterministic bf16 DDIM graph run against its fp32 run over as many evaluations
    det = rel_rms(p16(latents=x, num_inference_steps=evals, output_type="latent").float(),
                  p32(latents=x, num_inference_steps=evals, output_type="latent", use_graph=False))
    return dict(p32=p32, p16=p16, u16=u16, x=x, known=known, half=half, det=det)


def _fp32_eager_with_bf16_draws(ffhq, monkeypatch, seed):
    """The fp32 eager loop on the inputs of the bf16 run: a bf16 model draws its noise in bf16 (randn_tensor in the model's dtype),
    so the fp32 loop is made to draw the same values."""
    from afldm_amd.schedulers.schedule import Schedule
    from afldm_amd.utils import randn_tensor
    with monkeypatch.context() as mp:
        mp.setattr(Schedule, "draw_noise", lambda self, shape, generator, device, model_dtype:
                   randn_tensor(shape, generator=generator, device=device, dtype=torch.bfloat16))
        return ffhq["p32"].inpaint_latents(ffhq["known"], ffhq["half"], num_inference_steps=FN, eta=0.7, jump_length=FJ,
                                           jump_n_sample=FR, latents=ffhq["x"], generator=torch.Generator().manual_seed(seed),
                                           use_graph=False)


@pytest.mark.parametrize("branches", [1, 2])
def test_ffhq_bf16_graph_vs_fp32_eager(ffhq, monkeypatch, branches):
    from afldm_amd import trunk
    want = _fp32_eager_with_bf16_draws(ffhq, monkeypatch, 41)
    pipe = ffhq["p16"]
    if branches == 2:
        monkeypatch.setattr(trunk, "_BLOCKED", set(trunk._BLOCKED))
        monkeypatch.setenv("AFLDM_BRANCHES", "2")
        pipe = _ldm(ffhq["u16"])                                         # a pipeline of its own: the engine is made under the setting
    kw = dict(num_inference_steps=FN, eta=0.7, jump_length=FJ, jump_n_sample=FR, latents=ffhq["x"])
    got = pipe.inpaint_latents(ffhq["known"], ffhq["half"], generator=torch.Generator().manual_seed(41), **kw)
    (eng,) = pipe._repaint_engines.values()
    assert eng.branches == branches and got.dtype == torch.bfloat16
    err, det = rel_rms(got.float(), want), ffhq["det"]
    eager = pipe.inpaint_latents(ffhq["known"], ffhq["half"], generator=torch.Generator().manual_seed(41), use_graph=False, **kw)
    err_eager = rel_rms(eager.float(), want)
    print(f"[FFHQ RePaint (4, 2, 2) eta=0.7, 6 evaluations, batch 2, AFLDM_BRANCHES={branches}] bf16 rel-RMS vs the fp32 eager loop: "
          f"graph {err:.3e}, bf16 eager loop {err_eager:.3e}; bf16 DDIM graph vs fp32, 6 steps: {det:.3e}")
    assert err <= 1.5 * det, (err, det)
    s = ffhq["x"].shape[-1]
    assert torch.equal(got.float().cpu()[..., : s // 2], ffhq["known"].bfloat16().float()[..., : s // 2])


def test_ffhq_inpaint_end_to_end(ffhq):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from test_gpu_vae import build_vae
    vae, _, _ = build_vae(torch.float32)
    pipe = MyLDMPipeline(vae, ffhq["u16"], ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    s = ffhq["x"].shape[-1]
    S = 8 * s
    g = torch.Generator().manual_seed(9)
    image = F.interpolate(torch.rand(2, 3, 8, 8, generator=g) * 2 - 1, size=(S, S), mode="bicubic", align_corners=False).clamp(-1, 1)
    mask = torch.ones(1, 1, S, S)
    mask[..., S // 4: S // 2 + 3, S // 4: S // 2] = 0.0                   # (a hole whose lower edge is not on the latent grid)
    kw = dict(num_inference_steps=FN, jump_length=FJ, jump_n_sample=FR, eta=0.0)
    pt = pipe.inpaint(image, mask, generator=torch.Generator().manual_seed(2), output_type="pt", **kw)
    assert tuple(pt.shape) == (2, 3, S, S) and pt.dtype == torch.float32 and torch.isfinite(pt).all()
    keep = (mask == 1).expand_as(image)
    assert torch.equal(pt.cpu()[keep], image[keep])                       # composite: kept pixels are the input's, exactly
    assert not torch.equal(pt.cpu()[~keep], image[~keep])
    lat = pipe.inpaint(image, mask, generator=torch.Generator().manual_seed(2), output_type="latent", **kw)
    assert tuple(lat.shape) == (2, 4, s, s) and lat.dtype == torch.bfloat16
    # the latent mask is the block minimum: a latent is kept - and equals the encoded image - only where all 64 pixels are
    from afldm_amd import harness
    z0 = harness.vae_encode_mode(vae, image.cuda()).float().cpu()
    lm = (-F.max_pool2d(-mask, 8) == 1).expand_as(z0)
    assert int((~lm).sum()) == 2 * 4 * (s // 4 + 1) * (s // 4)
    assert torch.equal(lat.float().cpu()[lm], z0.bfloat16().float()[lm])
    raw = pipe.inpaint(image, mask, generator=torch.Generator().manual_seed(2), output_type="pt", composite=False, **kw)
    assert tuple(raw.shape) == (2, 3, S, S) and not torch.equal(raw.cpu()[keep], image[keep])
    assert torch.equal(raw.float().cpu()[~keep], pt.cpu()[~keep])         # the same sample, composited or not
    (arr,) = pipe.inpaint(image, mask, generator=torch.Generator().manual_seed(2), output_type="np", return_dict=False, **kw)
    assert arr.shape == (2, S, S, 3) and arr.min() >= 0.0 and arr.max() <= 1.0
    out = pipe.inpaint(image, mask, generator=torch.Generator().manual_seed(2), **kw)
    assert len(out.images) == 2 and out.images[0].size == (S, S)
    soft = pipe.inpaint(image, mask, generator=torch.Generator().manual_seed(2), output_type="latent", mask_mode="mean", **kw)
    assert tuple(soft.shape) == (2, 4, s, s) and not torch.equal(soft, lat)
