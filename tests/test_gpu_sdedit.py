"""Image-to-image sampling (SDEdit with a change map) on MI355X: afldm_sdedit_step / afldm_sdedit_step_flat through the C ABI
against the float64 restatement (tests/sdedit_oracle.py).

Shapes: the smallest at which each path can go wrong - [2, 4, 4, 4] (16-byte groups), [2, 3, 5, 3] (scalar, HW % 4 != 0),
[3, 4, 4, 4] with one map for the whole batch.  Bounds for fp32 against the oracle: rtol 2e-6, atol 2e-6 max|want| -
tests/test_gpu_repaint.py's kernel bound, and the fp32 chain (two multiply-adds into a clamp, three more) is no longer.  The oracle
compares the change map with the same fp32 threshold the kernel reads, so elements ON a threshold are part of every comparison."""
import itertools
import math

import pytest
import torch

import sdedit_oracle as so

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
INF = math.inf
# (p, q, lo, hi, a, b, c, k0, k1, thr, 0, 0)
ROWS = [
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.3, 0.8, 0.6, 0.75, 0.0, 0.0),      # no clip, draws, thr above the next row's
    (1.2, -0.5, -2.0, 2.0, 0.6, 0.3, 0.0, 0.9, 0.43, 0.5, 0.0, 0.0),                # a mid row: clip, c = 0, z read, thr = 1/2
    (1.0, -0.9, -1.0, 1.0, 0.9, 0.4, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0),                 # the last row: k0 = 1, k1 = 0, thr = 0
    (1.1, -0.4, -INF, INF, 0.8, 0.2, 0.25, 1.0, 0.0, 0.25, 0.0, 0.0),               # z not read, z_u read
]
LAST = 2
SHAPES = [(2, 4, 4, 4), (2, 3, 5, 3), (3, 4, 4, 4)]
LEVELS = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])


def bound(want):
    return dict(rtol=2e-6, atol=2e-6 * float(want.nan_to_num(posinf=0.0, neginf=0.0).abs().max()), equal_nan=True)


def kernel_inputs(dtype, shape, seed=29):
    """x, eps (as the kernel reads it), orig, the change map [B, 1, H, W] with every level - so values below, on and above every
    row's threshold - the fixed noise z and a [steps, 2 B, C, H, W] noise buffer a batch slice of which is passed."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x[0, 0, 0, :3] = torch.tensor([0.5, 2.5, -3.0])                      # inside and beyond the bounds of rows 1 and 2
    e = torch.randn(shape, generator=g).to(dtype).float()
    orig = torch.randn(shape, generator=g)
    z = torch.randn(shape, generator=g)
    one = LEVELS[torch.randint(0, 5, (1, 1, H, W), generator=g)]
    one[0, 0, 0, :3] = 1.0                                               # (the clamp probes are released elements)
    one.reshape(-1)[3:8] = LEVELS
    if B == 3:
        cmap = one.expand(B, 1, H, W).contiguous()                       # one map for the batch, broadcast on the host
    else:
        cmap = torch.cat([one] + [LEVELS[torch.randint(0, 5, (1, 1, H, W), generator=g)] for _ in range(B - 1)])
    big = torch.randn(len(ROWS), 2 * B, C, H, W, generator=g)
    return x, e, orig, cmap, z, big


def nhwc(e, dtype):
    return e.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)


# ------------------------------------------------------------------------------------------------ the engine form
@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, SHAPES)))
def test_sdedit_step_kernel(dtype, shape):
    from afldm_amd import ops
    B = shape[0]
    x, e, orig, cmap, z, big = kernel_inputs(dtype, shape)
    e_nhwc = nhwc(e, dtype)
    # NaN wherever a row does not read: the step's noise where c = 0, and (in a second z) the fixed noise where k1 = 0
    poisoned = big.clone()
    for s, row in enumerate(ROWS):
        if row[6] == 0.0:
            poisoned[s] = math.nan
    noise = poisoned.cuda()[:, B:]                                       # a batch slice of a larger buffer, as a branch passes it
    assert not noise.is_contiguous() and noise.stride(0) == 2 * x.numel()
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    og, mg, zg, znan = orig.cuda(), cmap.cuda(), z.cuda(), torch.full_like(z, math.nan).cuda()
    full = cmap.expand_as(x)
    for s, row in enumerate(ROWS):
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        xg = x.cuda()
        out = ops.sdedit_step(xg, e_nhwc, og, mg, zg if row[8] != 0.0 else znan, noise, coef, idx, advance=False, out=xg)   # aliased
        assert out.data_ptr() == xg.data_ptr() and int(idx.item()) == s
        got = out.cpu()
        want = so.sdedit_step(x, e, orig, cmap, z, big[s, B:], so.f32(row))
        assert torch.isfinite(got).all(), s                              # nothing of an unread buffer reached the output
        torch.testing.assert_close(got.double(), want, **bound(want))
        held = full <= so.f32(row)[9]
        assert 0 < int(held.sum()) < held.numel() and int((full == so.f32(row)[9]).sum()) > 0       # both sides, and ON the threshold
        if s == LAST:
            assert torch.equal(got[held], orig[held]) and torch.equal(held, full == 0)              # c = 0: the original, bit for bit
        # not aliased: x is left alone, the same bits come out
        xg = x.cuda()
        out2 = ops.sdedit_step(xg, e_nhwc, og, mg, zg, noise, coef, idx)
        assert out2.data_ptr() != xg.data_ptr() and torch.equal(out2.cpu(), got) and torch.equal(xg.cpu(), x)
        # no noise buffer at all (a schedule none of whose steps draws): fine wherever c = 0
        if row[6] == 0.0:
            assert torch.equal(ops.sdedit_step(x.cuda(), e_nhwc, og, mg, zg, None, coef, idx).cpu(), got)
    # advance: the kernel reads row 0, then the counter moves on; a second launch reads row 1
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    ops.sdedit_step(xg, e_nhwc, og, mg, zg, noise, coef, idx, advance=True, out=xg)
    ops.sdedit_step(xg, e_nhwc, og, mg, zg, noise, coef, idx, advance=True, out=xg)
    assert int(idx.item()) == 2
    first = so.sdedit_step(x, e, orig, cmap, z, big[0, B:], so.f32(ROWS[0]))
    want = so.sdedit_step(first, e, orig, cmap, z, None, so.f32(ROWS[1]))
    # two chained updates: the first one's 2e-6 passes through |a p| < 1 of row 1 and the second adds its own
    torch.testing.assert_close(xg.cpu().double(), want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, SHAPES[:2])))
def test_select_keeps_nan_and_inf_out_of_held_elements(dtype, shape):
    """NaN and Inf planted in x and eps: a held element is finite and within bound of k0 orig + k1 z (a blend would leak 0 * NaN);
    a released element is NaN.  A NaN in the change map compares false: that element takes the released branch."""
    from afldm_amd import ops
    x, e, orig, cmap, z, big = kernel_inputs(dtype, shape)
    B = shape[0]
    s = 1                                                                # thr = 1/2, c = 0
    row = so.f32(ROWS[s])
    full = cmap.expand_as(x).clone()
    held = full <= row[9]
    g = torch.Generator().manual_seed(5)
    bad_x, bad_e = torch.rand(shape, generator=g) < 0.3, torch.rand(shape, generator=g) < 0.3
    bad_x[0, 0, 0, :3] = False
    xb, eb = x.clone(), e.clone()
    xb[bad_x] = math.nan
    eb[bad_e] = math.nan
    eb[0, 0, -1, -1] = math.inf
    bad = torch.isnan(xb) | ~torch.isfinite(eb)
    assert int((bad & held).sum()) > 0 and int((bad & ~held).sum()) > 0 and int((~bad & ~held).sum()) > 0
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
    got = ops.sdedit_step(xb.cuda(), nhwc(eb, dtype), orig.cuda(), cmap.cuda(), z.cuda(), big.cuda()[:, B:], coef, idx).cpu()
    want_held = (row[7] * orig.double() + row[8] * z.double())
    assert torch.isfinite(got[held]).all()
    torch.testing.assert_close(got[held].double(), want_held[held], **bound(want_held))
    # released: x0 = clamp(p x + q eps) is NaN where either is (or clamps an Inf to a bound, and b * Inf stays Inf)
    assert not torch.isfinite(got[bad & ~held]).any() and torch.isfinite(got[~bad & ~held]).all()
    want = so.sdedit_step(xb, eb, orig, cmap, z, None, row)
    ok = ~bad
    torch.testing.assert_close(got[ok].double(), want[ok], **bound(want[ok]))
    # NaN in the change map: generated, also where the map would have held the element
    mb = cmap.clone()
    flip = held[:, :1] & (torch.rand(mb.shape, generator=g) < 0.5)
    mb[flip] = math.nan
    assert int(flip.sum()) > 0
    got = ops.sdedit_step(x.cuda(), nhwc(e, dtype), orig.cuda(), mb.cuda(), z.cuda(), None, coef, idx).cpu()
    want = so.sdedit_step(x, e, orig, mb, z, None, row)
    released = so.reverse_step(x, e, None, row)
    sel = flip.expand_as(x)
    assert torch.equal(want[sel], released[sel]) and torch.isfinite(got).all()
    torch.testing.assert_close(got.double(), want, **bound(want))


# ------------------------------------------------------------------------------------------------ the flat form
@pytest.mark.parametrize("shape", [(1, 1, 37, 1), (2, 1, 4, 4), (3, 1, 5, 5)])
def test_flat_form_is_the_engine_form_bit_for_bit(shape):
    """C = 1: NCHW and NHWC are one layout, and the map has x's shape, so both entries see the same memory.  n = 37: nine 16-byte
    groups and a scalar tail of one in the flat kernel, the scalar kernel in the engine form; n = 32: 16-byte groups in both;
    n = 75: groups and a tail of three."""
    from afldm_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, e, orig, z = [torch.randn(shape, generator=g) for _ in range(4)]
    cmap = LEVELS[torch.randint(0, 5, (B, 1, H, W), generator=g)]
    big = torch.randn(len(ROWS), B, C, H, W, generator=g)
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    nan = torch.full_like(x, math.nan).cuda()
    for s, row in enumerate(ROWS):
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        table = ops.sdedit_step(x.cuda(), e.reshape(B, H, W, C).cuda(), orig.cuda(), cmap.cuda(), z.cuda(), big.cuda(), coef, idx).cpu()
        zs = z.cuda() if row[8] != 0.0 else None
        zu = big[s].cuda() if row[6] != 0.0 else None
        xg = x.cuda()
        flat = ops.sdedit_step_flat(xg, e.cuda(), orig.cuda(), cmap.expand_as(x).contiguous().cuda(), zs, zu, so.f32(row), out=xg)
        assert flat.data_ptr() == xg.data_ptr()
        assert torch.equal(flat.cpu(), table), s
        want = so.sdedit_step(x, e, orig, cmap, z, big[s], so.f32(row))
        torch.testing.assert_close(table.double(), want, **bound(want))
        # a tensor the row does not read may hold anything
        out = ops.sdedit_step_flat(x.cuda(), e.cuda(), orig.cuda(), cmap.cuda(), zs if zs is not None else nan, zu if zu is not None else nan,
                                   so.f32(row))
        assert torch.equal(out.cpu(), table)
    with pytest.raises(ValueError):
        ops.sdedit_step_flat(x.cuda(), e.cuda(), orig.cuda(), cmap.cuda(), None, None, ROWS[0])     # k1 != 0 and c != 0 need tensors


@pytest.mark.parametrize("shape", [(2, 4, 4, 4), (1, 1, 37, 1)])
def test_start_row(shape):
    """x_start is the update under (p = q = 0, no clip, a = b = c = 0, k0, k1, thr = +inf): everything held, whatever x, eps and the
    map hold - the one formula the start and every held element share."""
    from afldm_amd import ops
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    g = torch.Generator().manual_seed(8)
    orig, z, junk = [torch.randn(shape, generator=g) for _ in range(3)]
    start = ffhq_ddim_scheduler().sdedit_start(8, 0.5)
    row = so.start_row(*start)
    want = so.x_start(orig, z, start)
    zero = torch.zeros(shape).cuda()
    got = ops.sdedit_step_flat(zero, zero, orig.cuda(), zero, z.cuda(), None, row).cpu()
    torch.testing.assert_close(got.double(), want, **bound(want))
    junk[0, 0, 0, 0] = math.nan
    maps = torch.rand(shape, generator=g) * 1e30
    again = ops.sdedit_step_flat(junk.cuda(), junk.cuda(), orig.cuda(), maps.cuda(), z.cuda(), None, row).cpu()
    assert torch.equal(again, got)


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_errors():
    from afldm_amd import _lib, ops
    lib = _lib.lib
    shape = (2, 4, 4, 4)
    x, e, orig, cmap, z, big = kernel_inputs(torch.float32, shape)
    xg, eg, og, mg, zg, ng = x.cuda(), nhwc(e, torch.float32), orig.cuda(), cmap.cuda(), z.cuda(), big.cuda()[:, 2:]
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    P, st, n = _lib.ptr, _lib.stream_ptr(), x.numel()
    ENULL, ESHAPE, EDTYPE = -5, -1, -2

    def call(**over):
        a = dict(x=P(xg), eps=P(eg), orig=P(og), cmap=P(mg), z=P(zg), noise=P(ng), stride=ng.stride(0), out=P(xg), coef=P(coef),
                 idx=P(idx), B=2, C=4, H=4, W=4, dtype=_lib.F32)
        a.update(over)
        return lib.afldm_sdedit_step(a["x"], a["eps"], a["orig"], a["cmap"], a["z"], a["noise"], a["stride"], a["out"], a["coef"],
                                     a["idx"], 0, a["B"], a["C"], a["H"], a["W"], a["dtype"], st)
    for name in ("x", "eps", "orig", "cmap", "z", "out", "coef", "idx"):
        assert call(**{name: None}) == ENULL, name
    for over in (dict(B=0), dict(C=-1), dict(H=0), dict(W=0), dict(stride=n - 1)):
        assert call(**over) == ESHAPE, over
    assert call(dtype=7) == EDTYPE
    assert b"sdedit" in lib.afldm_last_error()
    row = so.f32(ROWS[0])[:10]
    flat = [P(xg), P(xg), P(og), P(og), P(zg), P(zg), P(xg)]
    for i in (0, 1, 2, 3, 6):
        args = list(flat)
        args[i] = None
        assert lib.afldm_sdedit_step_flat(*args, *row, n, st) == ENULL, i
    for i in (4, 5):                                                     # z with k1 != 0, z_u with c != 0
        args = list(flat)
        args[i] = None
        assert lib.afldm_sdedit_step_flat(*args, *row, n, st) == ENULL, i
    assert lib.afldm_sdedit_step_flat(None, None, None, None, None, None, None, *row, 0, st) == ENULL
    assert lib.afldm_sdedit_step_flat(*flat, *row, 0, st) == 0          # nothing to do
    torch.cuda.synchronize()
    assert torch.equal(xg.cpu(), x)                                      # no refused call wrote anything
    # the wrappers: shapes (a batch-1 map is broadcast by the caller, not here), devices
    with pytest.raises(ValueError):
        ops.sdedit_step(xg, eg, og, mg[:1], zg, ng, coef, idx)
    with pytest.raises(ValueError):
        ops.sdedit_step(xg, eg, og[:1], mg, zg, ng, coef, idx)
    with pytest.raises(ValueError):
        ops.sdedit_step(xg, eg[:, :2].contiguous(), og, mg, zg, ng, coef, idx)
    with pytest.raises(ValueError):
        ops.sdedit_step_flat(xg, xg, og, mg, zg, zg, row)                # the map not expanded
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sdedit_step(x, eg, og, mg, zg, ng, coef, idx)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sdedit_step(xg, eg, og, cmap, zg, ng, coef, idx)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sdedit_step_flat(xg, xg, orig, og, zg, zg, row)
    with pytest.raises(RuntimeError):
        ops.sdedit_step(xg, eg.half(), og, mg, zg, ng, coef, idx)        # fp32 / bf16 only


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_tensors_take_the_scalar_path(dtype):
    """Tensors that start 4 bytes into their allocation (HW % 4 == 0 all the same) and a noise stride that is no multiple of 4: the
    launch falls back to scalar accesses and gives the bits of the aligned launch."""
    from afldm_amd import ops
    shape = (2, 4, 4, 4)
    x, e, orig, cmap, z, big = kernel_inputs(dtype, shape)
    n = x.numel()

    def off(t):
        buf = torch.zeros(t.numel() + 1, device="cuda")
        buf[1:].copy_(t.reshape(-1))
        v = buf[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    odd = torch.zeros(len(ROWS), n + 3, device="cuda")
    odd[:, :n].copy_(big[:, 2:].reshape(len(ROWS), n))
    odd_noise = odd[:, :n].view(len(ROWS), *shape)
    assert odd_noise.stride(0) == n + 3
    for s, row in enumerate(ROWS):
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        aligned = ops.sdedit_step(x.cuda(), nhwc(e, dtype), orig.cuda(), cmap.cuda(), z.cuda(), big.cuda()[:, 2:], coef, idx).cpu()
        for which in range(5):
            t = [x.cuda(), orig.cuda(), cmap.cuda(), z.cuda()]
            if which < 4:
                t[which] = off(t[which])
            noise = odd_noise if which == 4 else big.cuda()[:, 2:]
            got = ops.sdedit_step(t[0], nhwc(e, dtype), t[1], t[2], t[3], noise, coef, idx).cpu()
            assert torch.equal(got, aligned), (s, which)
        xo = off(x.cuda())
        assert torch.equal(ops.sdedit_step(xo, nhwc(e, dtype), orig.cuda(), cmap.cuda(), z.cuda(), None if row[6] == 0.0 else odd_noise, coef,
                                           idx, out=xo).cpu(), aligned)
        if dtype == torch.float32:
            fl = [off(v.cuda()) for v in (x, e, orig, cmap.expand_as(x).contiguous(), z, big[s, 2:])]
            ref = ops.sdedit_step_flat(x.cuda(), e.cuda(), orig.cuda(), cmap.expand_as(x).contiguous().cuda(), z.cuda(), big[s, 2:].cuda(),
                                       so.f32(row)).cpu()
            assert torch.equal(ops.sdedit_step_flat(*fl, so.f32(row)).cpu(), ref), s
