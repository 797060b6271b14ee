"""The plumbing launches of csrc/misc.hip on MI355X, per element: layout and weight packing, afldm_cast, the step
prologue, the masked metrics, the timestep embedding, SiLU and the DDIM update, against the float64 references, case
lists and derived tolerances of tests/plumbing_oracle.py (its docstring holds the derivations; the CPU side is
tests/test_plumbing_oracle_host.py).  Exact comparisons are on bit patterns or values with no tolerance; bounded ones
print their worst error over the bound.

Measured on one MI355X: this file (94 tests) and tests/test_gpu_fir_edges.py (95 tests) together run in 2.7 s of
pytest time in one process; no single test takes 0.5 s.

test_silu_fp32_against_float64[below_-87] found a defect in afldm_silu and is its regression test (its docstring)."""
import math

import pytest
import torch

import plumbing_oracle as po

pytestmark = pytest.mark.gpu
DTYPES = list(po.DTYPES)
IDS = ["fp32", "bf16"]


def _ops():
    from afldm_amd import ops
    return ops


def _raw():
    from afldm_amd import _lib
    return _lib


def _source(n, dtype):
    """Addressed fp32 values that `dtype` holds exactly (what to_nhwc / pack_weight read)."""
    return po.addressed(n, dtype).float()


# ------------------------------------------------------------------------------------------------ layout, packing
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", po.LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_addressed(shape, dtype):
    ops = _ops()
    B, C, H, W = shape
    x = _source(B * C * H * W, dtype).reshape(shape)
    y = ops.to_nhwc(x.cuda(), dtype)
    assert y.dtype == dtype and tuple(y.shape) == (B, H, W, C)
    po.assert_identical(y, po.nhwc_reference(x).to(dtype), f"to_nhwc {shape}", by_bits=True, names=("b", "h", "w", "c"))
    src = po.addressed(B * C * H * W, dtype).reshape(B, H, W, C)             # an NHWC tensor of its own addresses
    z = ops.to_nchw(src.cuda())
    assert z.dtype == torch.float32
    po.assert_identical(z, po.nchw_reference(src).float(), f"to_nchw {shape}", by_bits=True, names=("b", "c", "h", "w"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", po.PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_weight_addressed(shape, dtype):
    ops = _ops()
    w = _source(math.prod(shape), dtype).reshape(shape)
    got = ops.pack_weight(w.cuda(), dtype)
    want = po.pack_reference(w).to(dtype)
    assert got.dtype == dtype and got.shape == want.shape
    po.assert_identical(got, want, f"pack_weight {shape}", by_bits=True, names=("o", "kh", "kw", "i"))


def test_layout_rounding_probes():
    ops = _ops()
    p = po.rounding_probes()
    x = p.reshape(1, 2, 3, 5)
    po.assert_identical(ops.to_nhwc(x.cuda(), torch.bfloat16), po.expected_bf16(po.nhwc_reference(x)), "to_nhwc bf16 probes", by_bits=True)
    po.assert_identical(ops.to_nhwc(x.cuda(), torch.float32), po.nhwc_reference(x), "to_nhwc fp32 probes", by_bits=True)
    yb = po.expected_bf16(p).reshape(1, 3, 5, 2)
    po.assert_identical(ops.to_nchw(yb.cuda()), po.nchw_reference(yb).float(), "to_nchw bf16 probes", by_bits=True)
    po.assert_identical(ops.to_nchw(p.reshape(1, 3, 5, 2).cuda()), po.nchw_reference(p.reshape(1, 3, 5, 2)), "to_nchw fp32 probes", by_bits=True)
    w = p.reshape(3, 5, 1, 2)
    po.assert_identical(ops.pack_weight(w.cuda(), torch.bfloat16), po.expected_bf16(po.pack_reference(w)), "pack bf16 probes", by_bits=True)
    po.assert_identical(ops.pack_weight(w.cuda(), torch.float32), po.pack_reference(w), "pack fp32 probes", by_bits=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layout_out_forms_keep_canaries(dtype):
    ops = _ops()
    B, C, H, W = 2, 3, 5, 7
    n = B * C * H * W
    x = _source(n, dtype).reshape(B, C, H, W)
    buf, view = po.with_canaries((B, H, W, C), dtype, "cuda")
    assert ops.to_nhwc(x.cuda(), out=view).data_ptr() == view.data_ptr()
    po.assert_identical(view, po.nhwc_reference(x).to(dtype), "to_nhwc out=", by_bits=True)
    assert po.canaries_intact(buf, n)
    src = po.addressed(n, dtype).reshape(B, H, W, C)
    buf, view = po.with_canaries((B, C, H, W), torch.float32, "cuda")
    assert ops.to_nchw(src.cuda(), out=view).data_ptr() == view.data_ptr()
    po.assert_identical(view, po.nchw_reference(src).float(), "to_nchw out=", by_bits=True)
    assert po.canaries_intact(buf, n)


# ------------------------------------------------------------------------------------------------ afldm_cast
def _cast(src, dst, n, sd=None, dd=None):
    L = _raw()
    sd = L.DTYPE_CODE[src.dtype] if sd is None else sd
    dd = L.DTYPE_CODE[dst.dtype] if dd is None else dd
    rc = L.lib.afldm_cast(src.data_ptr(), sd, dst.data_ptr(), dd, n, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dst_dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("src_dtype", DTYPES, ids=IDS)
def test_cast_every_pair(src_dtype, dst_dtype):
    ok = _raw().ABI.constants["AFLDM_OK"]
    probes = po.rounding_probes() if src_dtype == torch.float32 else po.expected_bf16(po.rounding_probes())
    sources = [probes] + [po.addressed(n, src_dtype) for n in po.CAST_SIZES]
    for src in sources:
        n = src.numel()
        buf, view = po.with_canaries((n,), dst_dtype, "cuda")
        assert _cast(src.cuda(), view, n) == ok
        # torch's conversion is RNE for fp32 -> bf16, exact for bf16 -> fp32, the identity otherwise
        po.assert_identical(view, src.to(dst_dtype), f"cast {src_dtype} -> {dst_dtype} n={n}", by_bits=True)
        assert po.canaries_intact(buf, n), n


def test_cast_empty_and_unknown_dtype():
    L = _raw()
    ok, edtype = L.ABI.constants["AFLDM_OK"], L.ABI.constants["AFLDM_EDTYPE"]
    src = po.addressed(8, torch.float32).cuda()
    buf, view = po.with_canaries((8,), torch.float32, "cuda")
    assert _cast(src, view, 0) == ok                                         # n = 0: nothing is written
    assert bool((buf == -77.0).all())
    for sd, dd in ((7, L.F32), (L.BF16, -1), (2, 2)):
        assert _cast(src, view, 8, sd=sd, dd=dd) == edtype
        assert b"dtype" in L.lib.afldm_last_error()
        assert bool((buf == -77.0).all())
    assert _cast(src, view, 8) == ok                                         # the library goes on working
    po.assert_identical(view, src, "cast after a refusal", by_bits=True)


# ------------------------------------------------------------------------------------------------ step prologue
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("row_bytes", po.ROW_BYTES)
def test_select_step_row(row_bytes, dtype):
    ops = _ops()
    tvals, table = po.step_table(row_bytes, dtype)
    tv, tb = tvals.cuda(), table.cuda()
    per = table.shape[1]
    for pre in (False, True):
        for read in (0, 2, po.STEP_ROWS - 1):                                 # the first, a middle and the last row
            step = read - int(pre)                                            # (a pre-advancing loop starts at -1)
            row, t, after = po.step_row_reference(tvals, table, step, pre)
            assert after == read
            idx = torch.full((1,), step, dtype=torch.int32, device="cuda")
            t_out = torch.full((3,), -5.0, device="cuda")
            buf, view = po.with_canaries((per,), dtype, "cuda")
            ops.select_step_row(tv, idx, t_out[1:2], tb, view, pre_advance=pre)
            po.assert_identical(view, row, f"row of step {step} pre_advance={pre}", by_bits=True, names=("element",))
            assert t_out.tolist() == [-5.0, float(t), -5.0] and int(idx.item()) == after
            assert po.canaries_intact(buf, per)
            idx.fill_(step)
            t_out.fill_(-5.0)
            ops.select_timestep(tv, idx, t_out[1:2], pre_advance=pre)
            assert t_out.tolist() == [-5.0, float(t), -5.0] and int(idx.item()) == after


def test_select_step_row_refusals():
    """Rows that are not whole 16-byte chunks and a misaligned destination are refused before any launch."""
    L = _raw()
    ealign = L.ABI.constants["AFLDM_EALIGN"]
    tv = torch.tensor([9.0, 8.0, 7.0], device="cuda")
    idx = torch.ones(1, dtype=torch.int32, device="cuda")
    t_out = torch.full((1,), -5.0, device="cuda")
    table = po.addressed(3 * 8, torch.float32).reshape(3, 8).cuda()
    buf = torch.full((16,), -77.0, device="cuda")
    calls = [(buf[4:10], 24),                                                # a row of 24 bytes
             (buf[1:5], 16),                                                 # row_out one element past a 16-byte boundary
             (buf[4:8], 0)]
    for row_out, nbytes in calls:
        for pre in (0, 1):
            rc = L.lib.afldm_select_step_row(tv.data_ptr(), idx.data_ptr(), t_out.data_ptr(), pre, table.data_ptr(),
                                             row_out.data_ptr(), nbytes, L.stream_ptr())
            torch.cuda.synchronize()
            assert rc == ealign, (nbytes, pre, rc)
            assert bool((buf == -77.0).all()) and float(t_out.item()) == -5.0 and int(idx.item()) == 1
    rc = L.lib.afldm_select_step_row(tv.data_ptr(), idx.data_ptr(), t_out.data_ptr(), 0, table.data_ptr() + 4,
                                     buf[4:8].data_ptr(), 16, L.stream_ptr())   # a misaligned table
    torch.cuda.synchronize()
    assert rc == ealign and bool((buf == -77.0).all()) and float(t_out.item()) == -5.0 and int(idx.item()) == 1


# ------------------------------------------------------------------------------------------------ masked metrics
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", po.METRIC_SIZES)
def test_masked_metrics_exact(n, dtype):
    ops = _ops()
    a, b, m = po.metrics_case(n, dtype)
    got = ops.masked_metrics(a.cuda(), b.cuda(), m.cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 6)
    po.assert_identical(got.double(), po.metrics_reference(a, b, m), f"masked_metrics n={n}", names=("sample", "output"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_metrics_broadcast_mask(dtype):
    ops = _ops()
    a, b, _ = po.metrics_case(4 * 7 * 9, dtype, seed=5)
    a, b = a.reshape(3, 4, 7, 9), b.reshape(3, 4, 7, 9)
    m = (torch.rand(3, 1, 7, 9, generator=torch.Generator().manual_seed(6)) > 0.5).float()
    ref = po.metrics_reference(a, b, m)
    ref[:, 1] = m.double().reshape(3, -1).sum(1)                             # the mask's own shape is what is counted
    got = ops.masked_metrics(a.cuda(), b.cuda(), m.cuda())
    po.assert_identical(got.double(), ref, "masked_metrics broadcast mask", names=("sample", "output"))


# ------------------------------------------------------------------------------------------------ timestep embedding
def test_timestep_embedding_exact_properties():
    ops = _ops()
    t = po.emb_timesteps().cuda()
    for dim in po.EMB_WIDTHS:
        for shift in (0.0, 1.0):
            if dim == 2 and shift == 1.0:
                continue
            half = dim // 2
            hi = ops.timestep_embedding(t, dim, flip_sin_to_cos=True, freq_shift=shift)
            lo = ops.timestep_embedding(t, dim, flip_sin_to_cos=False, freq_shift=shift)
            po.assert_identical(lo[:, :half], hi[:, half:], f"sine half, dim {dim} shift {shift}", by_bits=True, names=("row", "k"))
            po.assert_identical(lo[:, half:], hi[:, :half], f"cosine half, dim {dim} shift {shift}", by_bits=True, names=("row", "k"))
            assert bool((hi[0, :half] == 1).all()) and bool((hi[0, half:] == 0).all())           # t = 0
            for flip, f32 in ((True, hi), (False, lo)):
                hb = ops.timestep_embedding(t, dim, flip_sin_to_cos=flip, freq_shift=shift, dtype=torch.bfloat16)
                po.assert_identical(hb, f32.cpu().to(torch.bfloat16), f"bf16 embedding, dim {dim} shift {shift} flip {flip}",
                                    by_bits=True, names=("row", "k"))


@pytest.mark.parametrize("dim,shift", [(d, s) for d in po.EMB_WIDTHS for s in (0.0, 1.0) if (d, s) != (2, 1.0)])   # 0 / 0 there
def test_timestep_embedding_against_float64(dim, shift):
    ops = _ops()
    t = po.emb_timesteps()
    for flip in (True, False):
        ref, a_abs = po.emb_reference(t, dim, flip=flip, freq_shift=shift)
        got = ops.timestep_embedding(t.cuda(), dim, flip_sin_to_cos=flip, freq_shift=shift)
        po.assert_within(got.cpu(), ref, po.emb_tolerance(a_abs), f"timestep_embedding dim {dim} shift {shift} flip {flip}")


# ------------------------------------------------------------------------------------------------ SiLU
SILU_SPLIT = -87.0          # below it 1 + exp(-x) leaves the range whose reciprocal is a normal fp32 number


@pytest.mark.parametrize("part", ["from_-87_up", "below_-87"])
def test_silu_fp32_against_float64(part):
    """The 4096-point grid on [-100, 100] and the six extra points, in two parts so that each reports its own worst
    figure: x >= -87, and x < -87 where exp2 overflows or its reciprocal is a denormal.

    The part below -87 is the regression test of a defect it found: with silu_f alone 94 of its 268 points were over the
    bound, the worst 86.09 times, at x = -87.3504 (got -0.0, float64 -1.0126e-36, bound 1.1763e-38).  From x = -87.35
    down 1 + exp2(-x log2 e) exceeds 2^126, the hardware reciprocal returns 0 for a denormal result, and the launch gave
    -0 where x / (1 + exp(-x)) is still a normal fp32 number (down to x = -91.9).  k_silu now evaluates x exp(x) below
    -87 (misc.hip, silu_full_range).  This pins afldm_silu; the fused kernels call silu_f itself and still return -0
    there."""
    ops = _ops()
    x = po.silu_points()
    x = x[x >= SILU_SPLIT] if part == "from_-87_up" else x[x < SILU_SPLIT]
    ref = po.silu_reference(x)
    got = ops.silu(x.cuda()).cpu()
    tol = po.silu_tolerance(x, ref)
    k = po.worst_over_bound(got, ref, tol)[1]
    print(f"silu fp32 {part}: worst at x = {float(x[k])!r}: got {float(got[k])!r}, float64 {float(ref[k])!r}, bound {float(tol[k])!r}")
    po.assert_within(got, ref, tol, f"silu fp32 {part} ({x.numel()} points)")


def test_silu_bf16_is_the_rounded_fp32_launch_and_specials():
    ops = _ops()
    xb = torch.cat([po.silu_points(), torch.tensor([math.inf, -math.inf, math.nan, 0.0, -0.0])]).to(torch.bfloat16)
    f32 = ops.silu(xb.float().cuda()).cpu()
    po.assert_identical(ops.silu(xb.cuda()), f32.to(torch.bfloat16), "silu bf16 vs rounded fp32 launch", by_bits=True, names=("point",))
    for v in (math.inf, -math.inf, math.nan):
        want = float(po.silu_reference(torch.tensor([v]))[0])
        for dtype in DTYPES:
            got = float(ops.silu(torch.tensor([v], dtype=dtype).cuda()).float().item())
            assert (math.isnan(want) and math.isnan(got)) or got == want, (v, dtype, got, want)


# ------------------------------------------------------------------------------------------------ DDIM
def _ddim_inputs(shape, dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    eps = torch.randn(shape, generator=g).to(dtype)                           # NCHW, as the kernel will read it
    coef = torch.tensor(po.DDIM_ROWS, dtype=torch.float32).reshape(-1)
    return x, eps, coef


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", po.DDIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ddim_step_against_float64(shape, dtype):
    ops = _ops()
    x, eps, coef = _ddim_inputs(shape, dtype)
    ref, scale = po.ddim_reference(x, eps, po.DDIM_ROWS[1])
    tol = po.ddim_tolerance(ref, scale)
    e_nhwc = po.nhwc_reference(eps).cuda()
    outs = []
    for advance in (False, True):
        idx = torch.ones(1, dtype=torch.int32, device="cuda")
        out = ops.ddim_step(x.cuda(), e_nhwc, coef.cuda(), idx, advance=advance)
        assert int(idx.item()) == 1 + int(advance)                           # and the update itself used row 1
        po.assert_within(out.cpu(), ref, tol, f"ddim_step {shape} {dtype} advance={advance}")
        outs.append(out.cpu())
    po.assert_identical(outs[1], outs[0], "advance changes the update", by_bits=True)
    idx = torch.ones(1, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    assert ops.ddim_step(xg, e_nhwc, coef.cuda(), idx, advance=True, out=xg).data_ptr() == xg.data_ptr()
    po.assert_identical(xg, outs[0], "x_prev aliasing x", by_bits=True, names=("b", "c", "h", "w"))
    assert int(idx.item()) == 2


@pytest.mark.parametrize("shape", po.DDIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ddim_step_flat_against_float64(shape):
    ops = _ops()
    x, eps, _ = _ddim_inputs(shape, torch.float32, seed=4)
    ref, scale = po.ddim_reference(x, eps, po.DDIM_ROWS[1])
    out = ops.ddim_step_flat(x.cuda(), eps.cuda(), po.DDIM_ROWS[1])
    po.assert_within(out.cpu(), ref, po.ddim_tolerance(ref, scale), f"ddim_step_flat {shape}")
    xg = x.cuda()
    ops.ddim_step_flat(xg, eps.cuda(), po.DDIM_ROWS[1], out=xg)
    po.assert_identical(xg, out, "flat x_prev aliasing x", by_bits=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 3, 5, 5), (1, 4, 1, 1), (1, 5, 363, 363)], ids=lambda s: "x".join(map(str, s)))
def test_ddim_step_gathers_eps_by_address(shape, dtype):
    """x = 0 and the row (1, 0, 0, 1): x_prev is eps itself, so the output names the NHWC element each NCHW position read."""
    ops = _ops()
    B, C, H, W = shape
    eps = po.addressed(B * C * H * W, dtype).reshape(B, H, W, C)
    coef = torch.tensor([po.DDIM_ROWS[0], po.DDIM_GATHER_ROW, po.DDIM_ROWS[2]], dtype=torch.float32).reshape(-1).cuda()
    idx = torch.ones(1, dtype=torch.int32, device="cuda")
    out = ops.ddim_step(torch.zeros(shape, device="cuda"), eps.cuda(), coef, idx)
    po.assert_identical(out, po.nchw_reference(eps).float(), f"ddim gather {shape}", names=("b", "c", "h", "w"))
