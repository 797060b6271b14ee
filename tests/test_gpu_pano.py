"""MultiDiffusion's kernels on MI355X (csrc/pano.hip): afldm_pano_step, afldm_window_fuse and afldm_window_crop against the float64
restatement of tests/pano_oracle.py on fp32-rounded coefficient rows, with eps in fp32 and bf16.

Bounds.  The allowed absolute error is not fixed in advance (tests/test_gpu_ilvr.py's construction).  It is the sum of
  (1) 2e-6 max|want| - test_sde_step_kernel's bound for the elementwise fp32 chain - and
  (2) twice the max-abs error of the same weighted means taken in fp32 by torch on the CPU (ascending k, as the kernel) against
      float64 on the same fp32 inputs, each mean weighed by the coefficient it enters the update with: 2 (|b| err(mean x0) +
      |d| err(mean eps)); the factor 2 covers fmaf against multiply-then-add and the one division.
Both terms and the kernel's error are printed.  With one window of weight 1 term (2) is 0.  What is exact is asserted with
torch.equal: the windows are the crops of the canvas, one window of weight 1 is afldm_sde_step, aliased and separate outputs, a
canvas alone or second of two, an unread noise row full of NaN, and where a NaN in eps arrives."""
import itertools
import math

import pytest
import torch

import pano_oracle as po

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
INF = math.inf
# (p, q, lo, hi, a, b, d, c)
ROWS = [
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.0, 0.7, 0.5, 0.0),         # DDIM-shaped: no clip, c = 0 (the noise row is not read)
    (1.0, -0.9, -1.0, 1.0, 0.0, 0.55, 0.1, 0.2),                  # clipped, with noise
    (1.0, -0.4, -INF, INF, 0.4, 0.55, 0.2, 0.3),                  # a != 0
]
# (P, C, S, Hc, Wc, stride_y, stride_x, circular_x)
GEOMS = [
    (2, 4, 4, 4, 11, 3, 3, False),          # the last window flush with a short gap
    (1, 3, 4, 6, 7, 2, 2, False),           # a 2-D grid, odd extents, odd C (one element per thread)
    (2, 4, 4, 4, 9, 3, 3, True),            # wrap
    (1, 4, 5, 5, 5, 5, 5, False),           # a single window
    (2, 4, 16, 16, 40, 8, 8, False),        # the tiny UNet's plane
    (1, 4, 32, 32, 64, 16, 16, True),       # the FFHQ plane
]


def f32(row):
    return [float(v) for v in torch.tensor(row, dtype=torch.float64).to(torch.float32)]


def geometry(shape):
    from afldm_amd.panorama import Geometry
    P, C, S, Hc, Wc, sy, sx, circ = shape
    return Geometry.grid(Hc, Wc, S, sy, sx, circular_x=circ)


def inputs(dtype, shape, seed=23):
    """x, eps as NCHW fp32 holding what the kernel reads (rounded to dtype), one noise row per ROWS entry, a non-uniform wt."""
    P, C, S, Hc, Wc = shape[:5]
    g = geometry(shape)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, Hc, Wc, generator=gen)
    x[0, 0, 0, :4] = torch.tensor([0.5, -0.5, 0.75, -3.0])                 # on and beyond the clip of row 1
    e = torch.randn(P * g.nwin, C, S, S, generator=gen).to(dtype).float()
    z = torch.randn(len(ROWS), P, C, Hc, Wc, generator=gen)
    wt = torch.rand(S, S, generator=gen) + 0.25
    return g, x, e, z, wt


def nhwc(e, dtype):
    return e.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)


def mean_bound(values, wt, g):
    """max |fp32 mean - float64 mean| of fp32 window values on the CPU."""
    v = values.float()
    return float((po.fuse(v, wt, g, torch.float32).double() - po.fuse(v, wt, g)).abs().max())


def step_bound(x, e, z, wt, g, row, label):
    r = f32(row)
    want, wins = po.pano_step(x, e, z, wt, g, r)
    t1 = 2e-6 * float(want.abs().max())
    t2 = 2.0 * (abs(r[5]) * mean_bound(po.x0_windows(x, e, g, r), wt, g) + abs(r[6]) * mean_bound(e, wt, g))
    print(f"    {label}: bound terms (1) {t1:.2e} + (2) {t2:.2e}  (max|want| {t1 / 2e-6:.2f})")
    return want, wins, t1 + t2


def launch(x, e_dev, z_dev, wt_dev, g, s, alias=True):
    from afldm_amd import ops
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    out, wins = ops.pano_step(xg, e_dev, z_dev, wt_dev, g, coef, idx, advance=False, out=xg if alias else None)
    assert (out.data_ptr() == xg.data_ptr()) == alias and int(idx.item()) == s
    if not alias:
        assert torch.equal(xg.cpu(), x)                                   # the input is left alone
    return out.cpu(), wins.cpu()


# ------------------------------------------------------------------------------------------------ afldm_pano_step
@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, GEOMS)))
def test_pano_step_kernel(dtype, shape):
    g, x, e, z, wt = inputs(dtype, shape)
    e_dev, ones = nhwc(e, dtype), torch.ones(g.S, g.S)
    # NaN in every noise row its coefficient row does not read: the kernel must not load it (0 * NaN is not 0)
    poisoned = z.clone()
    for s, row in enumerate(ROWS):
        if row[7] == 0.0:
            poisoned[s] = math.nan
    z_dev = poisoned.cuda()
    print()
    for s, row, w in [(s, row, ones) for s, row in enumerate(ROWS)] + [(1, ROWS[1], wt)]:        # ... and once with a random wt > 0
        uniform = w is ones
        label = f"{str(dtype)[6:]} {shape} row {s}" + ("" if uniform else " random wt")
        want, want_wins, tol = step_bound(x, e, z[s], w, g, row, label)
        got, wins = launch(x, e_dev, z_dev, w.cuda(), g, s)
        assert torch.isfinite(got).all()
        err = float((got.double() - want).abs().max())
        print(f"        kernel max-abs error {err:.2e} of {tol:.2e} allowed")
        assert err <= tol, (s, err, tol)
        assert torch.equal(wins, po.crop(got, g))                         # the next UNet input is the canvas, cropped
        got2, wins2 = launch(x, e_dev, z_dev, w.cuda(), g, s, alias=False)
        assert torch.equal(got2, got) and torch.equal(wins2, wins)


@pytest.mark.parametrize("dtype,S", list(itertools.product(DTYPES, [5, 16])))
def test_single_window_is_the_sde_step_bit_for_bit(dtype, S):
    """One window of weight 1 (GEOMS[3]'s plane, S = 5) is afldm_sde_step: the same bits.  That kernel has two forms which differ
    in the last bit - at S = 5 one element per thread with every product and sum rounded on its own, which is the arithmetic of
    afldm_pano_step; at S = 16 its 16-byte form, which the compiler contracts into fma - so at S = 16 the two agree within that
    kernel's own bound (test_sde_step_kernel's 2e-6) and not bit for bit."""
    from afldm_amd import ops
    shape = (2, 4, S, S, S, S, S, False)
    g, x, e, z, _ = inputs(dtype, shape)
    assert g.nwin == 1
    e_dev, z_dev, ones = nhwc(e, dtype), z.cuda(), torch.ones(S, S, device="cuda")
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    for s in range(len(ROWS)):
        got, wins = launch(x, e_dev, z_dev, ones, g, s)
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        sde = ops.sde_step(x.cuda(), e_dev, z_dev, coef, idx).cpu()
        assert torch.equal(wins, got)
        if S == 5:
            assert torch.equal(got, sde), s
        else:
            torch.testing.assert_close(got, sde, rtol=2e-6, atol=2e-6 * float(sde.abs().max()))


@pytest.mark.parametrize("shape", [GEOMS[0], GEOMS[2], GEOMS[4]])
def test_canvas_bits_do_not_depend_on_the_batch(shape):
    """Every canvas of a batch of two, run alone (P = 1), gives the bits it gives inside the batch."""
    g, x, e, z, wt = inputs(torch.float32, shape)
    assert x.shape[0] == 2
    n = g.nwin
    for s in range(len(ROWS)):
        both, wins = launch(x, nhwc(e, torch.float32), z.cuda(), wt.cuda(), g, s)
        for i in (0, 1):
            one, w1 = launch(x[i:i + 1], nhwc(e[i * n:(i + 1) * n], torch.float32), z[:, i:i + 1].contiguous().cuda(), wt.cuda(), g, s)
            assert torch.equal(one, both[i:i + 1]) and torch.equal(w1, wins[i * n:(i + 1) * n]), (s, i)


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, [GEOMS[1], GEOMS[2], GEOMS[4]])))
def test_a_nan_in_eps_reaches_its_element_and_nothing_else(dtype, shape):
    P, C, S = shape[:3]
    g, x, e, z, wt = inputs(dtype, shape)
    clean, clean_wins = launch(x, nhwc(e, dtype), z.cuda(), wt.cuda(), g, 2)
    k, ch, u, v = g.nwin - 1, C - 1, 1, S - 1                            # the last window of the last canvas
    bad = e.clone()
    bad[(P - 1) * g.nwin + k, ch, u, v] = math.nan
    got, wins = launch(x, nhwc(bad, dtype), z.cuda(), wt.cuda(), g, 2)
    oy, ox = g.corners()[k]
    Y, X = (oy + u) % g.Hc, (ox + v) % g.Wc
    where = torch.zeros_like(got, dtype=torch.bool)
    where[P - 1, ch, Y, X] = True
    assert torch.equal(torch.isnan(got), where)
    assert torch.equal(torch.isnan(wins), po.crop(where, g)) and int(torch.isnan(wins).sum()) >= 1
    assert torch.equal(got.nan_to_num(7.0), torch.where(where, torch.full_like(got, 7.0), clean))
    # without noise (c = 0) a noise buffer is not needed at all
    from afldm_amd import ops
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    a, _ = ops.pano_step(x.cuda(), nhwc(e, dtype), None, wt.cuda(), g, coef, idx)
    b, _ = launch(x, nhwc(e, dtype), z.cuda(), wt.cuda(), g, 0)
    assert torch.equal(a.cpu(), b)


def test_pano_step_advances_like_the_other_updates():
    from afldm_amd import ops
    g, x, e, z, wt = inputs(torch.float32, GEOMS[0])
    e_dev, z_dev, w_dev = nhwc(e, torch.float32), z.cuda(), wt.cuda()
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    for _ in range(2):
        ops.pano_step(xg, e_dev, z_dev, w_dev, g, coef, idx, advance=True, out=xg)
    assert int(idx.item()) == 2
    y = x
    for s in (0, 1):
        y, _ = launch(y, e_dev, z_dev, w_dev, g, s)
    assert torch.equal(xg.cpu(), y)


def test_refusals_leave_the_outputs_alone():
    from afldm_amd import ops
    from afldm_amd._lib import AfldmError
    from afldm_amd.panorama import Geometry
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad = [
        (Geometry(4, 11, 4, (0,), (0, 7)), "no window covers"),                         # x = 4 .. 6 are in no window
        (Geometry(4, 11, 4, (0,), (0, 4, 8)), "leaves"),                                # 8 + 4 > 11 on an axis that does not wrap
        (Geometry(4, 11, 4, (0,), (0, 4, -1)), "leaves"),
        (Geometry(4, 9, 4, (0,), (0, 3, 9), False, True), "leaves"),                    # a wrapping axis takes origins below its extent
        (Geometry(4, 9, 4, (0,), (0, 5), False, True), "no window covers"),             # x = 4 and 0: wrap does not close this gap
        (Geometry(4, 34, 4, (0,), tuple(range(0, 32, 2)) + (30,)), "origins"),          # 17 windows on an axis
        (Geometry(4, 3, 4, (0,), (0,)), "canvas"),                                      # S > extent
    ]
    for g, what in bad:
        P, C = 1, 4
        canvas = torch.zeros(P, C, g.Hc, g.Wc, device="cuda")
        eps = torch.zeros(P * g.nwin, g.S, g.S, C, device="cuda")
        out, wins = torch.full_like(canvas, 3.0), torch.full((P * g.nwin, C, g.S, g.S), 3.0, device="cuda")
        ones = torch.ones(g.S, g.S, device="cuda")
        with pytest.raises(AfldmError, match=what):
            ops.pano_step(canvas, eps, None, ones, g, coef, idx, advance=True, out=out, windows_out=wins)
        with pytest.raises(AfldmError, match=what):
            ops.window_fuse(wins, ones, g, out=out)
        with pytest.raises(AfldmError, match=what):
            ops.window_crop(canvas, g, out=wins)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()) and bool((wins == 3.0).all()) and int(idx.item()) == 0
    g = geometry(GEOMS[0])
    with pytest.raises(ValueError):                                       # a weight plane of another size
        ops.window_fuse(torch.zeros(g.nwin, 2, 4, 4, device="cuda"), torch.ones(5, 5, device="cuda"), g)
    with pytest.raises(ValueError):
        ops.window_crop(torch.zeros(1, 2, 4, 12, device="cuda"), g)


# ------------------------------------------------------------------------------------------------ afldm_window_fuse / _crop
@pytest.mark.parametrize("shape", GEOMS)
def test_window_crop_is_exact_and_fuse_inverts_it(shape):
    from afldm_amd import ops
    g, x, e, z, wt = inputs(torch.float32, shape)
    wins = ops.window_crop(x.cuda(), g)
    assert torch.equal(wins.cpu(), po.crop(x, g))
    print()
    for w, name in ((torch.ones(g.S, g.S), "ones"), (wt, "random wt")):
        # fuse(crop(canvas)) is the canvas, within the bound of a mean of equal values
        back = ops.window_fuse(wins, w.cuda(), g).cpu()
        tol = 2e-6 * float(x.abs().max()) + 2.0 * mean_bound(po.crop(x, g), w, g)
        err = float((back - x).abs().max())
        print(f"    {shape} {name}: fuse(crop(x)) - x max-abs {err:.2e} of {tol:.2e} allowed")
        assert err <= tol
        # independent windows against float64
        want = po.fuse(e, w, g)
        t1, t2 = 2e-6 * float(want.abs().max()), 2.0 * mean_bound(e, w, g)
        got = ops.window_fuse(e.cuda(), w.cuda(), g).cpu()
        err = float((got.double() - want).abs().max())
        print(f"    {shape} {name}: fuse max-abs error {err:.2e} of (1) {t1:.2e} + (2) {t2:.2e} allowed")
        assert err <= t1 + t2


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, [GEOMS[0], GEOMS[2]])))
def test_window_fuse_in_pixel_units_with_a_feather(dtype, shape):
    """The pixel-space blend: 32 x 32 windows (S r = 32, r = 8) in the model dtype under the triangular feather."""
    from afldm_amd import ops
    from afldm_amd.panorama import feather
    g = geometry(shape).scaled(8)
    assert g.S == 32 and g.Wc == 8 * shape[4]
    P, C = shape[0], 3
    gen = torch.Generator().manual_seed(5)
    wins = torch.randn(P * g.nwin, C, 32, 32, generator=gen).to(dtype)
    t = torch.tensor(feather(32))
    wt = torch.outer(t, t)
    want = po.fuse(wins.float(), wt, g)
    t1, t2 = 2e-6 * float(want.abs().max()), 2.0 * mean_bound(wins.float(), wt, g)
    got = ops.window_fuse(wins.cuda(), wt.cuda(), g).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (P, C, g.Hc, g.Wc)
    err = float((got.double() - want).abs().max())
    print(f"\n    {str(dtype)[6:]} {shape} x 8: feathered fuse max-abs error {err:.2e} of (1) {t1:.2e} + (2) {t2:.2e} allowed")
    assert err <= t1 + t2
