"""ILVR reference-guided sampling on the graph-replayed engine (MI355X): afldm_ilvr_step / afldm_ilvr_step_flat against a float64
torch restatement, MyLDMPipeline.ilvr_latents on replayed graphs against its own eager loop (same generator, same draws), against
the "sde" sampler and DDIM where it is never conditioned, against the CPU oracle UNet driven by a float64 loop, the invariants of
an ILVR sampler with a projection for phi, and FFHQ-size bf16 runs.

Bounds.  Kernel: the allowed absolute error is not fixed in advance.  It is the sum of
  (1) 2e-6 max|want| - test_sde_step_kernel's bound for the elementwise fp32 chain - and
  (2) twice the max-abs error of the same two plane products (Lh d Lw^T) computed by torch on the CPU in fp32 against float64 on
      the same inputs; the factor 2 covers a different but fixed summation order.
Both terms and the kernel's error are printed.  The shift test and the projection invariants hold within that same bound.  The
invariants are evaluated with the fp32 matrix the kernel is given, which is a projection only to its rounding: an update computed
exactly from it already misses both by (3) max|L (L d L^T) L^T - L d L^T| (float64 arithmetic, fp32 matrix; ~1e-7 of max|d|), a
property of the input and not of the kernel, so (3) is added there and printed.  Graph against eager: rel-RMS 1e-5, fp32 against the oracle: 1e-3
(tests/test_gpu_repaint.py's and test_gpu_sde.py's bounds for the same comparisons).  bf16: no number fixed in advance - the graph
run may differ from the fp32 eager loop on the same draws by 1.5x what the deterministic bf16 DDIM graph run differs from its
fp32 run over as many evaluations."""
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
# (p, q, lo, hi, a, b, c, k0, k1, w, 0, 0)
ROWS = [
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.3, 0.8, 0.6, 1.0, 0.0, 0.0),       # guided, both slots, no clip
    (1.0, -0.9, -INF, INF, 0.9, 0.4, 0.0, 0.9, 0.43, 1.0, 0.0, 0.0),                 # guided, c = 0: z_u not read
    (1.0, -0.4, -1.0, 1.0, 0.95, 0.2, 0.25, 1.0, 0.0, 1.0, 0.0, 0.0),                # guided, k1 = 0: z_k not read; clip
    (1.2, -0.5, -INF, INF, 0.6, 0.3, 0.2, 0.8, 0.6, 0.0, 0.0, 0.0),                  # w = 0: the plain stochastic step
]
SHAPES = [(3, 4, 16), (2, 3, 5), (2, 4, 32), (1, 2, 64)]          # 16-byte path / odd plane, scalar path / FFHQ plane / LDS bound


def f32(row):
    return [float(v) for v in torch.tensor(row, dtype=torch.float64).to(torch.float32)]


def reads(row):
    """(z_k is read, z_u is read) for this row."""
    return row[9] != 0.0 and row[8] != 0.0, row[6] != 0.0


def parts(x, e, ref, zs, row):
    """(xp, yk) in float64 on the fp32-rounded row; a slot is not looked at where the kernel does not read it."""
    p, q, lo, hi, a, b, c, k0, k1, w = f32(row)[:10]
    x, e, ref = x.double(), e.double(), ref.double()
    zk, zu = [z.double() if on else torch.zeros_like(x) for z, on in zip(zs, (k1 != 0.0, c != 0.0))]
    return a * torch.clamp(p * x + q * e, lo, hi) + b * e + c * zu, k0 * ref + k1 * zk


def phi(d, Lh, Lw):
    return Lh.double() @ d @ Lw.double().T


def torch_ilvr(x, e, ref, zs, Lh, Lw, row):
    xp, yk = parts(x, e, ref, zs, row)
    w = f32(row)[9]
    return xp if w == 0.0 else xp + w * phi(yk - xp, Lh, Lw)


def bound(x, e, ref, zs, Lh, Lw, row, label=None):
    """The allowed absolute error for this row: (1) + (2) of the module docstring, measured on the planes without a NaN."""
    xp, yk = parts(x, e, ref, zs, row)
    want = torch_ilvr(x, e, ref, zs, Lh, Lw, row)
    t1 = 2e-6 * float(want.nan_to_num().abs().max())
    if f32(row)[9] == 0.0:
        return t1, t1, 0.0
    d32 = (yk - xp).nan_to_num().float()
    t2 = 2.0 * float((phi(d32.double(), Lh, Lw) - (Lh @ d32 @ Lw.T).double()).abs().max())
    if label:
        print(f"    {label}: bound terms (1) {t1:.2e} + (2) {t2:.2e}  (max|want| {t1 / 2e-6:.2f}: (2) is {t2 / (t1 / 2e-6):.1e} of it)")
    return t1 + t2, t1, t2


def ideal(S, factor=2):
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    return ilvr_filter(S, factor).float()


def matrices(kind, S):
    if kind == "ideal":
        L = ideal(S)
        return L, L
    g = torch.Generator().manual_seed(S)
    return tuple(torch.randn(S, S, generator=g) / math.sqrt(S) for _ in range(2))             # not symmetric, Lh != Lw


def kernel_inputs(dtype, shape):
    B, C, S = shape
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, C, S, S, generator=g)
    x[0, 0, 0, :4] = torch.tensor([0.5, -0.5, 0.75, -3.0])              # on and beyond the clip of row 2
    x[B - 1, C - 1, 1, 3] = math.nan
    e = torch.randn(B, C, S, S, generator=g).to(dtype).float()           # what the kernel reads
    ref = torch.randn(B, C, S, S, generator=g)
    big = torch.randn(len(ROWS), 2, 2 * B, C, S, S, generator=g)
    return x, e, ref, big


def nan_plane_only(got, shape, whole_plane):
    B, C, S = shape
    nan = torch.isnan(got)
    if whole_plane:
        return bool(nan[B - 1, C - 1].all()) and int(nan.sum()) == S * S
    return bool(nan[B - 1, C - 1, 1, 3]) and int(nan.sum()) == 1


CASES = [(dt, sh, "ideal") for dt, sh in itertools.product(DTYPES, SHAPES)] + [(torch.float32, (3, 4, 16), "random"),
                                                                               (torch.float32, (2, 3, 5), "random")]


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype,shape,mats", CASES)
def test_ilvr_step_kernel(dtype, shape, mats):
    from afldm_amd import ops
    B, C, S = shape
    x, e, ref, big = kernel_inputs(dtype, shape)
    Lh, Lw = matrices(mats, S)
    e_nhwc = e.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)
    # NaN in every slot the row does not read: the kernel must not load it (0 * NaN is not 0)
    poisoned = big.clone()
    for s, row in enumerate(ROWS):
        for j, on in enumerate(reads(row)):
            if not on:
                poisoned[s, j] = math.nan
    noise = poisoned.cuda()[:, :, B:]                                    # a batch slice of a larger buffer, as a branch passes it
    assert not noise.is_contiguous() and noise.stride(1) == 2 * x.numel()
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    rg, Lhg = ref.cuda(), Lh.cuda()
    Lwg = Lhg if mats == "ideal" else Lw.cuda()                          # the pipeline passes the same pointer twice
    nan_ref, nan_L = torch.full_like(rg, math.nan), torch.full_like(Lhg, math.nan)
    print()
    for s, row in enumerate(ROWS):
        guided = row[9] != 0.0
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        xg = x.cuda()
        # w = 0: ref, z_k and the filter are not read either
        args = (rg, noise, Lhg, Lwg) if guided else (nan_ref, noise, nan_L, nan_L)
        out = ops.ilvr_step(xg, e_nhwc, *args, coef, idx, advance=False, out=xg)                    # x_out aliases x
        assert out.data_ptr() == xg.data_ptr() and int(idx.item()) == s
        zs = big[s, :, B:]
        want = torch_ilvr(x, e, ref, zs, Lh, Lw, row)
        got = out.cpu()
        # x's NaN: over exactly its own plane where the plane is filtered, its own pixel where it is not
        assert nan_plane_only(got, shape, guided), s
        tol, _, _ = bound(x, e, ref, zs, Lh, Lw, row, f"{str(dtype)[6:]} {shape} {mats} row {s}")
        err = float((got.double() - want).nan_to_num().abs().max())
        print(f"        kernel max-abs error {err:.2e} of {tol:.2e} allowed")
        assert err <= tol, (s, err, tol)
        if s == 3:
            assert torch.equal(torch.isnan(got), torch.isnan(want))
        # not aliased: x is left alone, the result is the same bits
        xg = x.cuda()
        out2 = ops.ilvr_step(xg, e_nhwc, *args, coef, idx)
        assert out2.data_ptr() != xg.data_ptr() and torch.equal(out2.cpu().nan_to_num(7.0), got.nan_to_num(7.0))
        assert torch.equal(xg.cpu().nan_to_num(7.0), x.nan_to_num(7.0))
    # advance: the kernel reads row 0, then the counter moves on; a second launch reads row 1 - the same bits as two launches
    # that are told their rows
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    ops.ilvr_step(xg, e_nhwc, rg, noise, Lhg, Lwg, coef, idx, advance=True, out=xg)
    ops.ilvr_step(xg, e_nhwc, rg, noise, Lhg, Lwg, coef, idx, advance=True, out=xg)
    assert int(idx.item()) == 2
    yg = x.cuda()
    for s in (0, 1):
        ops.ilvr_step(yg, e_nhwc, rg, noise, Lhg, Lwg, coef, torch.full((1,), s, dtype=torch.int32, device="cuda"), out=yg)
    assert torch.equal(xg.cpu().nan_to_num(7.0), yg.cpu().nan_to_num(7.0))


@pytest.mark.parametrize("shape", [(2, 4, 32), (2, 3, 5), (4, 4, 16)])
def test_ilvr_step_batch_slices_are_bit_identical(shape):
    """A plane's result does not depend on B, the grid or the batch slice it arrived in: two halves of a batch, each as a
    slice of the whole buffers, against one call on the whole."""
    from afldm_amd import ops
    B, C, S = shape
    x, e, ref, big = kernel_inputs(torch.float32, shape)
    x = x.nan_to_num(0.25)
    L = ideal(S).cuda()
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    xg, eg, rg, ng = x.cuda(), e.permute(0, 2, 3, 1).contiguous().cuda(), ref.cuda(), big.cuda()[:, :, :B].contiguous()
    h = B // 2
    for s in range(len(ROWS)):
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        whole = ops.ilvr_step(xg, eg, rg, ng, L, L, coef, idx)
        halves = [ops.ilvr_step(xg[i:i + h], eg[i:i + h], rg[i:i + h], ng[:, :, i:i + h], L, L, coef, idx) for i in (0, h)]
        assert torch.equal(torch.cat(halves), whole), s
        assert torch.isfinite(whole).all()


@pytest.mark.parametrize("shape", [(2, 4, 32), (2, 3, 5)])
def test_ilvr_step_commutes_with_a_circular_shift(shape):
    """L is circulant: rolling every input by (3, 5) rolls the output.  The sums then take their terms in another order, so
    the two agree within the kernel's bound, not bit for bit."""
    from afldm_amd import ops
    B, C, S = shape
    x, e, ref, big = kernel_inputs(torch.float32, shape)
    x = x.nan_to_num(0.25)
    Lc = ideal(S)
    L = Lc.cuda()
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()

    def roll(t):
        return torch.roll(t, (3, 5), (-2, -1)).contiguous()

    def run(x, e, ref, zs, s):
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        return ops.ilvr_step(x.cuda(), e.permute(0, 2, 3, 1).contiguous().cuda(), ref.cuda(), zs.cuda(), L, L, coef, idx).cpu()
    for s, row in enumerate(ROWS):
        zs = big[:, :, B:].contiguous()
        a, b = roll(run(x, e, ref, zs, s)), run(roll(x), roll(e), roll(ref), roll(zs), s)
        tol = bound(x, e, ref, zs[s], Lc, Lc, row)[0]
        err = float((a - b).abs().max())
        print(f"[shift (3, 5), {shape}, row {s}] max-abs difference {err:.2e} of {tol:.2e} allowed")
        assert err <= tol
        if row[9] == 0.0:
            assert torch.equal(a, b)


@pytest.mark.parametrize("shape,mats", [(sh, "ideal") for sh in SHAPES] + [((3, 4, 16), "random")])
def test_ilvr_step_flat_kernel(shape, mats):
    from afldm_amd import ops
    B, C, S = shape
    x, e, ref, big = kernel_inputs(torch.float32, shape)
    Lh, Lw = matrices(mats, S)
    Lhg, Lwg = Lh.cuda(), Lw.cuda()
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    nan = torch.full_like(x, math.nan).cuda()
    nan_L = torch.full_like(Lhg, math.nan)
    for s, row in enumerate(ROWS):
        guided = row[9] != 0.0
        zs = [big[s, j, B:].contiguous().cuda() if on else None for j, on in enumerate(reads(row))]
        xg = x.cuda()
        out = ops.ilvr_step_flat(xg, e.cuda(), ref.cuda(), zs, Lhg, Lwg, row, out=xg)
        assert out.data_ptr() == xg.data_ptr()
        got = out.cpu()
        want = torch_ilvr(x, e, ref, big[s, :, B:], Lh, Lw, row)
        assert nan_plane_only(got, shape, guided), s
        tol, _, _ = bound(x, e, ref, big[s, :, B:], Lh, Lw, row)
        err = float((got.double() - want).nan_to_num().abs().max())
        print(f"[flat {shape} {mats} row {s}] max-abs error {err:.2e} of {tol:.2e} allowed")
        assert err <= tol
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        table = ops.ilvr_step(x.cuda(), e.permute(0, 2, 3, 1).contiguous().cuda(), ref.cuda(), big.cuda()[:, :, B:], Lhg, Lwg, coef, idx)
        assert float((got.double() - table.cpu().double()).nan_to_num().abs().max()) <= 2 * tol
        # whatever the row does not read may hold anything
        out = ops.ilvr_step_flat(x.cuda(), e.cuda(), ref.cuda() if guided else nan, [z if z is not None else nan for z in zs],
                                 Lhg if guided else nan_L, Lwg if guided else nan_L, row)
        assert torch.equal(out.cpu().nan_to_num(7.0), got.nan_to_num(7.0))
    with pytest.raises(ValueError):
        ops.ilvr_step_flat(x.cuda(), e.cuda(), ref.cuda(), [None, None], Lhg, Lwg, ROWS[0])


@pytest.mark.parametrize("shape", [(3, 4, 16), (2, 4, 32), (2, 3, 5)])
def test_ilvr_projection_invariants(shape):
    """With a projection for phi, a guided row takes the low band from the noised reference and leaves the proposal's high
    band alone: L x_out L^T = L yk L^T and x_out - L x_out L^T = xp - L xp L^T."""
    from afldm_amd import ops
    B, C, S = shape
    x, e, ref, big = kernel_inputs(torch.float32, shape)
    x = x.nan_to_num(0.25)
    L = ideal(S)
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    for s, row in enumerate(ROWS[:3]):
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        zs = big[s, :, B:]
        got = ops.ilvr_step(x.cuda(), e.permute(0, 2, 3, 1).contiguous().cuda(), ref.cuda(), big.cuda()[:, :, B:], L.cuda(), L.cuda(),
                            coef, idx).cpu().double()
        xp, yk = parts(x, e, ref, zs, row)
        low = phi(yk - xp, L, L)
        defect = float((phi(low, L, L) - low).abs().max())                # (3): the fp32 matrix is a projection to this
        tol = bound(x, e, ref, zs, L, L, row)[0]
        lo_err = float((phi(got, L, L) - phi(yk, L, L)).abs().max())
        hi_err = float(((got - phi(got, L, L)) - (xp - phi(xp, L, L))).abs().max())
        print(f"[projection {shape} row {s}] low band {lo_err:.2e}, high band {hi_err:.2e} of {tol + defect:.2e} allowed "
              f"(kernel bound {tol:.2e} + L L - L defect {defect:.2e})")
        assert lo_err <= tol + defect and hi_err <= tol + defect


def test_ilvr_shape_refusal():
    """No kernel for S = 65 or H != W: the library says so before any launch, and ops raises."""
    from afldm_amd import ops
    from afldm_amd._lib import AfldmError
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    for H, W in ((65, 65), (16, 8), (8, 16), (1, 1)):
        x = torch.zeros(1, 2, H, W, device="cuda")
        noise = torch.zeros(len(ROWS), 2, 1, 2, H, W, device="cuda")
        Lh, Lw = torch.eye(H, device="cuda"), torch.eye(W, device="cuda")
        out = torch.full_like(x, 3.0)
        with pytest.raises(AfldmError, match="plane"):
            ops.ilvr_step(x, torch.zeros(1, H, W, 2, device="cuda"), x.clone(), noise, Lh, Lw, coef, idx, out=out)
        with pytest.raises(AfldmError, match="plane"):
            ops.ilvr_step_flat(x, x.clone(), x.clone(), [x.clone(), x.clone()], Lh, Lw, ROWS[0], out=out)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()) and int(idx.item()) == 0
    x = torch.zeros(1, 2, 16, 16, device="cuda")
    with pytest.raises(ValueError):                                      # a matrix of another size
        ops.ilvr_step_flat(x, x.clone(), x.clone(), [x.clone(), x.clone()], torch.eye(8, device="cuda"), torch.eye(16, device="cuda"),
                           ROWS[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ilvr_step_flat(x.cpu(), x.cpu(), x.cpu(), [None, None], torch.eye(16), torch.eye(16), ROWS[2])


# ------------------------------------------------------------------------------------------------ tiny UNet
N = 6


@pytest.fixture(scope="module")
def tiny():
    unet, cfg, sd = build("tiny", torch.float32)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ref = 0.8 * torch.randn(2, 4, 16, 16, generator=g)
    return dict(unet=unet, cfg=cfg, sd=sd, pipe=_ldm(unet), x=x, ref=ref)


@pytest.mark.parametrize("eta,range_t,kind", [(eta, rt, kind) for (eta, rt) in [(1.0, 0), (0.7, 300)] for kind in ("cpu", "cuda", "list")])
def test_tiny_graph_vs_eager_loop(tiny, eta, range_t, kind):
    pipe, x, ref = tiny["pipe"], tiny["x"], tiny["ref"]
    kw = dict(down_factor=2, range_t=range_t, num_inference_steps=N, eta=eta, latents=x)
    ga, gb, gc = _gens(kind, 11), _gens(kind, 11), _gens(kind, 11)
    a = pipe.ilvr_latents(ref, generator=ga, **kw)
    (key,) = pipe._ilvr_engines
    eng = pipe._ilvr_engines[key]
    assert eng.schedule.kind == "ilvr" and tuple(eng.noise.shape) == (N, 2, 2, 4, 16, 16) and tuple(eng.filter.shape) == (16, 16)
    assert sum(r[9] for r in eng.schedule.rows) == (N if range_t == 0 else sum(t > range_t for t in eng.schedule.timesteps))
    assert "_engines" not in pipe.__dict__ or key not in pipe._engines
    b = pipe.ilvr_latents(ref, generator=gb, use_graph=False, **kw)
    err = rel_rms(a, b)
    print(f"[tiny ILVR N={N} factor 2 eta={eta} range_t={range_t}, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe.ilvr_latents(ref, generator=gc, **kw))                                # seeded: bit-identical
    assert pipe._ilvr_engines[key] is eng
    # another reference and another cut-off: the same engine and graphs, and still the eager loop's result
    graphs = (eng.graph, eng.graph_multi)
    ref2 = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(5))
    kw2 = dict(kw, down_factor=4)
    ga, gb = _gens(kind, 12), _gens(kind, 12)
    a2 = pipe.ilvr_latents(ref2, generator=ga, **kw2)
    assert pipe._ilvr_engines[key] is eng and (eng.graph, eng.graph_multi) == graphs and graphs[0] is not None
    err2 = rel_rms(a2, pipe.ilvr_latents(ref2, generator=gb, use_graph=False, **kw2))
    print(f"    second reference and cut-off on the cached engine: rel-RMS {err2:.2e}")
    assert err2 <= 1e-5 and rel_rms(a2, a) > 1e-2


def test_tiny_never_conditioned_is_the_plain_sampler(tiny):
    pipe, x, ref = tiny["pipe"], tiny["x"], tiny["ref"]
    # range_t above every timestep: every row has w = 0, the launch is the stochastic step and the draws are the "sde" sampler's
    a = pipe.ilvr_latents(ref, range_t=1000, num_inference_steps=N, eta=0.7, latents=x, generator=torch.Generator().manual_seed(1))
    sde = pipe(latents=x, num_inference_steps=N, eta=0.7, generator=torch.Generator().manual_seed(1), output_type="latent")
    err = rel_rms(a, sde)
    print(f"[tiny ILVR range_t=1000, eta=0.7] vs the 'sde' sampler rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    b = pipe.ilvr_latents(ref, range_t=1000, num_inference_steps=N, eta=0.0, latents=x, generator=torch.Generator().manual_seed(1))
    ddim = pipe(latents=x, num_inference_steps=N, output_type="latent")
    err = rel_rms(b, ddim)
    print(f"[tiny ILVR range_t=1000, eta=0] vs DDIM {N} steps rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    eng = pipe._ilvr_engines[next(iter(pipe._ilvr_engines))]
    with pytest.raises(ValueError):
        eng.run(x, draw=lambda: x)                                        # no known=(ref, L)
    with pytest.raises(ValueError):
        eng.run(x, draw=lambda: x, known=(ref, torch.eye(8)))             # a filter of another size
    with pytest.raises(ValueError):
        eng.run(x, draw=lambda: x, known=(ref[:1], torch.eye(16)))


def test_tiny_low_band_is_the_reference(tiny):
    pipe, x, ref = tiny["pipe"], tiny["x"], tiny["ref"]
    L = ideal(16, 2)
    kw = dict(down_factor=2, range_t=0, num_inference_steps=N, latents=x)
    for use_graph in (True, False):
        a = pipe.ilvr_latents(ref, generator=torch.Generator().manual_seed(1), use_graph=use_graph, **kw).cpu().double()
        b = pipe.ilvr_latents(ref, generator=torch.Generator().manual_seed(2), use_graph=use_graph, **kw).cpu().double()
        lo = rel_rms(phi(a, L, L), phi(ref.double(), L, L))
        hi = rel_rms(a - phi(a, L, L), b - phi(b, L, L))
        print(f"[tiny ILVR factor 2, use_graph={use_graph}] low band vs the reference's rel-RMS {lo:.2e}; high band, seed 1 vs 2 {hi:.2e}")
        assert lo <= 1e-5 and rel_rms(phi(b, L, L), phi(ref.double(), L, L)) <= 1e-5
        assert hi > 1e-2
    # phi given as a matrix: the same sample as the factor that builds it
    c = pipe.ilvr_latents(ref, phi=L, generator=torch.Generator().manual_seed(1), **kw)
    assert rel_rms(c, a) <= 1e-5


def test_tiny_vs_oracle(tiny):
    """N = 6, eta = 1, factor 2: the oracle UNet on the CPU under a float64 loop over the schedule's rows, drawing the same noise
    (z_k, then z_u) from the same CPU generator."""
    from oracle import unet as ou
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe, x, ref = tiny["pipe"], tiny["x"], tiny["ref"]
    got = pipe.ilvr_latents(ref, down_factor=2, num_inference_steps=N, eta=1.0, latents=x, generator=torch.Generator().manual_seed(31))
    sched = ffhq_ddim_scheduler().ilvr_schedule(N, 1.0, 0)
    gen = torch.Generator().manual_seed(31)
    L = ilvr_filter(16, 2).float().double()                               # the matrix the kernel is given
    lat, r64 = x.double(), ref.double()
    for k, (t, row) in enumerate(zip(sched.timesteps, sched.rows)):
        p, q, lo, hi, a, b, c, k0, k1, w = row[:10]
        eps = ou.unet_forward(tiny["sd"], tiny["cfg"], lat.float(), t).double()
        zk = torch.randn(x.shape, generator=gen).double() if 0 in sched.slots(k) else 0.0
        zu = torch.randn(x.shape, generator=gen).double() if 1 in sched.slots(k) else 0.0
        xp = a * torch.clamp(p * lat + q * eps, lo, hi) + b * eps + c * zu
        lat = xp + w * (L @ ((k0 * r64 + k1 * zk) - xp) @ L.T)
    err = rel_rms(got, lat)
    print(f"[tiny ILVR N=6 eta=1 factor 2] fp32 rel-RMS vs the oracle loop {err:.3e}")
    assert err <= 1e-3, err


# ------------------------------------------------------------------------------------------------ FFHQ size, bf16
FN = 6


@pytest.fixture(scope="module")
def ffhq():
    u32, _, _ = build("ffhq", torch.float32)
    u16, _, _ = build("ffhq", torch.bfloat16)
    s = u32.config.sample_size
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 4, s, s, generator=g)
    ref = 0.8 * torch.randn(2, 4, s, s, generator=g)
    p32, p16 = _ldm(u32), _ldm(u16)
    # the yardstick: the deterministic bf16 DDIM graph run against its fp32 run over as many evaluations
    det = rel_rms(p16(latents=x, num_inference_steps=FN, output_type="latent").float(),
                  p32(latents=x, num_inference_steps=FN, output_type="latent", use_graph=False))
    return dict(p32=p32, p16=p16, u16=u16, x=x, ref=ref, det=det)


@pytest.mark.parametrize("branches", [1, 2])
def test_ffhq_bf16_graph_vs_fp32_eager(ffhq, monkeypatch, branches):
    from afldm_amd import trunk
    from afldm_amd.schedulers.schedule import Schedule
    from afldm_amd.utils import randn_tensor
    kw = dict(down_factor=4, num_inference_steps=FN, eta=1.0, latents=ffhq["x"])
    # the fp32 eager loop on the draws of the bf16 run: a bf16 model draws its noise in bf16
    with monkeypatch.context() as mp:
        mp.setattr(Schedule, "draw_noise", lambda self, shape, generator, device, model_dtype:
                   randn_tensor(shape, generator=generator, device=device, dtype=torch.bfloat16))
        want = ffhq["p32"].ilvr_latents(ffhq["ref"], generator=torch.Generator().manual_seed(41), use_graph=False, **kw)
    pipe = ffhq["p16"]
    if branches == 2:
        monkeypatch.setattr(trunk, "_BLOCKED", set(trunk._BLOCKED))
        monkeypatch.setenv("AFLDM_BRANCHES", "2")
        pipe = _ldm(ffhq["u16"])                                         # a pipeline of its own: the engine is made under the setting
    got = pipe.ilvr_latents(ffhq["ref"], generator=torch.Generator().manual_seed(41), **kw)
    (eng,) = pipe._ilvr_engines.values()
    assert eng.branches == branches and got.dtype == torch.bfloat16
    err, det = rel_rms(got.float(), want), ffhq["det"]
    eager = pipe.ilvr_latents(ffhq["ref"], generator=torch.Generator().manual_seed(41), use_graph=False, **kw)
    err_eager = rel_rms(eager.float(), want)
    print(f"[FFHQ ILVR factor 4 eta=1, {FN} evaluations, batch 2, AFLDM_BRANCHES={branches}] bf16 rel-RMS vs the fp32 eager loop: "
          f"graph {err:.3e}, bf16 eager loop {err_eager:.3e}; bf16 DDIM graph vs fp32, {FN} steps: {det:.3e}")
    assert err <= 1.5 * det, (err, det)


def test_ffhq_ilvr_end_to_end(ffhq):
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
    pt = pipe.ilvr(image, down_factor=4, num_inference_steps=4, generator=torch.Generator().manual_seed(2), output_type="pt")
    assert tuple(pt.shape) == (2, 3, S, S) and torch.isfinite(pt).all()
    lat = pipe.ilvr(image, down_factor=4, num_inference_steps=4, generator=torch.Generator().manual_seed(2), output_type="latent")
    assert tuple(lat.shape) == (2, 4, s, s) and lat.dtype == torch.bfloat16 and torch.isfinite(lat.float()).all()
    out = pipe.ilvr(image, down_factor=4, num_inference_steps=4, generator=torch.Generator().manual_seed(2))
    assert len(out.images) == 2 and out.images[0].size == (S, S)
