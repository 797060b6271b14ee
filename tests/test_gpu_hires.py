"""The high-resolution update on MI355X (csrc/hires.hip: afldm_hires_step and afldm_hires_windows, through ops.hires_step /
ops.hires_windows) against the float64 restatement of tests/hires_oracle.py on fp32-rounded coefficient rows, with eps in fp32 and
bf16, a uniform and a random window weight.

Bound.  Not fixed in advance; per case the sum of
  (1) 2e-6 max|want| - the sibling tests' figure for an elementwise fp32 chain of this length;
  (2) 2 (1 - r)(1 - g) (|a| err(mean x0) + |b| err(mean eps)), err(mean .) being test_gpu_pano.mean_bound: the same weighted means
      taken in fp32 by torch on the CPU (ascending k, as the kernel) against float64;
  (3) 2 |f| err(L out L^T): the same plane product taken in fp32 by torch on the CPU against float64 (test_gpu_ilvr's construction;
      the factor 2 covers a different but fixed summation order).
The canvas and the local windows do not pass the filter and are held to (1) + (2); the dilated windows to (1) + (2) + (3).  All
terms and the kernel's errors are printed.  What is exact is asserted with torch.equal: the local windows are the crops of the
canvas, with f = 0 the dilated windows its sub-lattices, with g = 0 and r = 0 the canvas and the local windows are
afldm_pano_repaint_step's with nothing kept, aliased and separate outputs, a canvas alone or second of two, afldm_hires_windows
against the step's windows, inputs a row does not read full of NaN, where a NaN in a local eps arrives, and that a refusal
writes nothing."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import hires_oracle as ho
import pano_oracle as po
from test_gpu_pano import f32, mean_bound, nhwc

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
INF = math.inf
# (p, q, lo, hi, a, b, c, k0, k1, r, g, f)
ROWS = [
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.2, 0.8, 0.6, 0.3, 0.4, 0.7),      # every term on
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.2, 0.8, 0.6, 0.3, 0.0, 0.7),      # g = 0: the dilated eps is not read
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.2, 0.8, 0.6, 0.0, 0.4, 0.7),      # r = 0: ref and eps_ref are not read
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.2, 0.8, 0.6, 0.3, 0.4, 0.0),      # f = 0: Lh and Lw are not read
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.0, 0.8, 0.6, 0.3, 0.4, 0.7),      # c = 0: the noise is not read
    (1.0, -0.9, -1.0, 1.0, 0.55, 0.1, 0.2, 0.8, 0.6, 0.3, 0.4, 1.0),               # a finite clip; f = 1: the views fully filtered
    (1 / 0.9, -0.3 / 0.9, -INF, INF, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.05, 0.0),     # the last evaluation: (..., 1, 0, 0, g, 0)
    (1.0, -0.9, -1.0, 1.0, 0.55, 0.1, 0.2, 0.8, 0.6, 0.0, 0.0, 0.7),               # g = r = 0 (afldm_pano_repaint_step's ground), c != 0
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.0, 0.8, 0.6, 0.0, 0.0, 0.0),      # ... and with nothing but the local windows read
]
# (S, scale, stride, C, P)
GEOMS = [
    (4, 2, 2, 3, 2),           # odd C
    (8, 2, 4, 4, 3),
    (5, 3, 2, 2, 1),           # an odd plane of 15, 36 + 9 windows
    (16, 4, 16, 4, 1),         # 64 x 64: the LDS bound, 16 + 16 windows
    (32, 2, 16, 4, 2),         # the FFHQ case, 9 + 4 windows
]


def geometry(shape):
    from afldm_amd.panorama import Geometry
    S, s, stride = shape[:3]
    return Geometry.grid(S * s, S * s, S, stride, stride)


def lowpass_matrix(shape):
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    return ilvr_filter(shape[0] * shape[1], shape[1]).float()


_INPUTS = {}


def inputs(dtype, shape, seed=31):
    """x, ref, eps_ref as NCHW fp32, eps NCHW fp32 holding what the kernel reads (rounded to dtype), one noise row per ROWS entry, a
    non-uniform wt and the fp32 low-pass.  Made once per (dtype, shape) and never written to."""
    if (dtype, shape) not in _INPUTS:
        S, s, _, C, P = shape
        g = geometry(shape)
        H, NW = S * s, g.nwin + s * s
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(P, C, H, H, generator=gen)
        x[0, 0, 0, :4] = torch.tensor([0.5, -0.5, 0.75, -3.0])             # on and beyond the clip of row 5
        e = torch.randn(P * NW, C, S, S, generator=gen).to(dtype).float()
        ref, eps_ref = torch.randn(P, C, H, H, generator=gen), torch.randn(P, C, H, H, generator=gen)
        z = torch.randn(len(ROWS), P, C, H, H, generator=gen)
        wt = torch.rand(S, S, generator=gen) + 0.25
        _INPUTS[dtype, shape] = (g, x, e, ref, eps_ref, z, wt, lowpass_matrix(shape))
    return _INPUTS[dtype, shape]


def poisoned(shape, s, e, ref, eps_ref, z, L):
    """NaN in everything row s does not read: the kernel must not load it (0 * NaN is not 0)."""
    row = ROWS[s]
    g, scale = geometry(shape), shape[1]
    e, ref, eps_ref, z, L = e.clone(), ref.clone(), eps_ref.clone(), z.clone(), L.clone()
    if row[10] == 0.0:
        e.reshape(-1, g.nwin + scale * scale, *e.shape[1:])[:, g.nwin:] = math.nan
    if row[9] == 0.0:
        ref[:], eps_ref[:] = math.nan, math.nan
    if row[6] == 0.0:
        z[s] = math.nan
    if row[11] == 0.0:
        L[:] = math.nan
    return e, ref, eps_ref, z, L


def step_bound(shape, x, e, ref, eps_ref, z, wt, L, row, label):
    g, scale = geometry(shape), shape[1]
    r = f32(row)
    want, wins = ho.hires_step(x, e, ref, eps_ref, z, wt, L, g, scale, r)
    t1 = 2e-6 * max(float(want.abs().max()), float(wins.abs().max()))
    loc = ho.split(e, g, scale)[0]
    t2 = 2.0 * abs(1.0 - r[9]) * abs(1.0 - r[10]) * (abs(r[4]) * mean_bound(po.x0_windows(x, loc, g, r), wt, g)
                                                     + abs(r[5]) * mean_bound(loc, wt, g))
    t3 = 0.0
    if r[11] != 0.0:
        t3 = 2.0 * abs(r[11]) * float((ho.lowpass(want, L) - ho.lowpass(want.float(), L, torch.float32)).abs().max())
    print(f"    {label}: bound terms (1) {t1:.2e} + (2) {t2:.2e} + (3) {t3:.2e}  (max|want| {t1 / 2e-6:.2f})")
    return want, wins, t1 + t2, t1 + t2 + t3


def launch(shape, x, e_dev, ref, eps_ref, z_dev, wt, L, s, alias=True, advance=False):
    from afldm_amd import ops
    g, scale = geometry(shape), shape[1]
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
    xg, Lg = x.cuda(), L.cuda()
    out, wins = ops.hires_step(xg, e_dev, ref.cuda(), eps_ref.cuda(), z_dev, wt.cuda(), Lg, Lg, g, scale, coef, idx, advance=advance,
                               out=xg if alias else None)
    assert (out.data_ptr() == xg.data_ptr()) == alias and int(idx.item()) == s + int(advance)
    if not alias:
        assert torch.equal(xg.cpu(), x)                                   # the input is left alone
    return out.cpu(), wins.cpu()


# ------------------------------------------------------------------------------------------------ afldm_hires_step
@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, GEOMS)))
def test_hires_step_kernel(dtype, shape):
    from afldm_amd import ops
    g, x, e, ref, eps_ref, z, wt, L = inputs(dtype, shape)
    scale, ones = shape[1], torch.ones(g.S, g.S)
    print()
    for s, w in [(s, ones) for s in range(len(ROWS))] + [(0, wt), (5, wt)]:           # ... and a random wt > 0
        label = f"{str(dtype)[6:]} {shape} row {s}" + ("" if w is ones else " random wt")
        want, want_wins, tol, tol_d = step_bound(shape, x, e, ref, eps_ref, z[s], w, L, ROWS[s], label)
        pe, pref, peps, pz, pL = poisoned(shape, s, e, ref, eps_ref, z, L)
        got, wins = launch(shape, x, nhwc(pe, dtype), pref, peps, pz.cuda(), w, pL, s)
        assert torch.isfinite(got).all() and torch.isfinite(wins).all()
        err = float((got.double() - want).abs().max())
        loc, dil = ho.split(wins, g, scale)
        wloc, wdil = ho.split(want_wins, g, scale)
        err_d = float((dil.double() - wdil).abs().max())
        print(f"        kernel max-abs error: canvas {err:.2e} of {tol:.2e} allowed, dilated windows {err_d:.2e} of {tol_d:.2e}")
        assert err <= tol and err_d <= tol_d, (s, err, tol, err_d, tol_d)
        assert torch.equal(loc, po.crop(got, g))                          # the local windows are the canvas, cropped
        if ROWS[s][11] == 0.0:
            assert torch.equal(dil, ho.views(got, scale))                 # f = 0: plain sub-lattices
        # the tail alone, on the canvas the step wrote, gives the step's windows
        alone = ops.hires_windows(got.cuda(), pL.cuda(), pL.cuda(), f32(ROWS[s])[11], g, scale).cpu()
        assert torch.equal(alone, wins)
        # a separate output; and with finite values in place of the NaN nobody reads, the same bits
        got2, wins2 = launch(shape, x, nhwc(pe, dtype), pref, peps, pz.cuda(), w, pL, s, alias=False)
        assert torch.equal(got2, got) and torch.equal(wins2, wins)
        got3, wins3 = launch(shape, x, nhwc(e, dtype), ref, eps_ref, z.cuda(), w, L, s)
        assert torch.equal(got3, got) and torch.equal(wins3, wins)
    # noise = None where no row that runs reads it
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    a, wa = ops.hires_step(x.cuda(), nhwc(e, dtype), ref.cuda(), eps_ref.cuda(), None, wt.cuda(), L.cuda(), L.cuda(), g, scale, coef, idx)
    b, wb = launch(shape, x, nhwc(e, dtype), ref, eps_ref, z.cuda(), wt, L, 4)
    assert torch.equal(a.cpu(), b) and torch.equal(wa.cpu(), wb)


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, [GEOMS[0], GEOMS[1], GEOMS[2], GEOMS[4]])))
def test_without_the_global_terms_it_is_the_outpainting_step_with_nothing_kept(dtype, shape):
    """g = 0 and r = 0: the canvas and the local windows are afldm_pano_repaint_step's under a zero mask, finite known content,
    u0 = 1 and u1 = 0 - bit for bit, with one element per thread there (odd C) and with four."""
    from afldm_amd import ops
    g, x, e, ref, eps_ref, z, wt, L = inputs(dtype, shape)
    S, scale, _, C, P = shape
    loc_e = ho.split(e, g, scale)[0].contiguous()
    for s in (7, 8):
        got, wins = launch(shape, x, nhwc(e, dtype), ref, eps_ref, z.cuda(), wt, L, s)
        row = ROWS[s][:9] + (1.0, 0.0, 0.0)
        coef = torch.tensor(row, dtype=torch.float32).cuda()
        idx = torch.zeros(1, dtype=torch.int32, device="cuda")
        noise = torch.zeros(1, 3, P, C, S * scale, S * scale)
        noise[0, 0], noise[0, 1] = eps_ref, z[s]
        want, want_wins = ops.pano_repaint_step(x.cuda(), nhwc(loc_e, dtype), ref.cuda(), torch.zeros(P, 1, S * scale, S * scale).cuda(),
                                                noise.cuda(), wt.cuda(), g, coef, idx)
        assert torch.equal(got, want.cpu()) and torch.equal(ho.split(wins, g, scale)[0], want_wins.cpu()), s


@pytest.mark.parametrize("shape", [GEOMS[0], GEOMS[4]])
def test_canvas_bits_do_not_depend_on_the_batch(shape):
    """Every canvas of a batch of two, run alone (P = 1), gives the bits it gives inside the batch."""
    g, x, e, ref, eps_ref, z, wt, L = inputs(torch.float32, shape)
    assert x.shape[0] == 2
    n = g.nwin + shape[1] ** 2
    one = shape[:4] + (1,)
    for s in (0, 5):
        both, wins = launch(shape, x, nhwc(e, torch.float32), ref, eps_ref, z.cuda(), wt, L, s)
        for i in (0, 1):
            alone, w1 = launch(one, x[i:i + 1], nhwc(e[i * n:(i + 1) * n], torch.float32), ref[i:i + 1], eps_ref[i:i + 1],
                               z[:, i:i + 1].contiguous().cuda(), wt, L, s)
            assert torch.equal(alone, both[i:i + 1]) and torch.equal(w1, wins[i * n:(i + 1) * n]), (s, i)


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, [GEOMS[0], GEOMS[1], GEOMS[2]])))
def test_a_nan_in_a_local_eps_reaches_its_element_its_copies_and_its_planes_dilated_views(dtype, shape):
    S, scale, _, C, P = shape
    g, x, e, ref, eps_ref, z, wt, L = inputs(dtype, shape)
    NW = g.nwin + scale * scale
    k = g.nwin - 1                                                       # the last local window of the last canvas
    oy, ox = g.corners()[k]
    ch, u, v = C - 1, 1, S - 1
    bad = e.clone()
    bad[(P - 1) * NW + k, ch, u, v] = math.nan
    for s in (0, 3):                                                     # f != 0, f == 0
        clean, clean_wins = launch(shape, x, nhwc(e, dtype), ref, eps_ref, z.cuda(), wt, L, s)
        got, wins = launch(shape, x, nhwc(bad, dtype), ref, eps_ref, z.cuda(), wt, L, s)
        where = torch.zeros_like(got, dtype=torch.bool)
        where[P - 1, ch, oy + u, ox + v] = True
        assert torch.equal(torch.isnan(got), where)
        assert torch.equal(got.nan_to_num(7.0), torch.where(where, torch.full_like(got, 7.0), clean))
        loc, dil = ho.split(wins, g, scale)
        assert torch.equal(torch.isnan(loc), po.crop(where, g)) and int(torch.isnan(loc).sum()) >= 1
        plane = torch.zeros_like(where)
        plane[P - 1, ch] = True
        assert torch.equal(torch.isnan(dil), ho.views(plane if ROWS[s][11] != 0.0 else where, scale))
        assert torch.equal(wins.nan_to_num(7.0), torch.where(torch.isnan(wins), torch.full_like(wins, 7.0), clean_wins))


def test_hires_step_advances_like_the_other_updates():
    shape = GEOMS[0]
    g, x, e, ref, eps_ref, z, wt, L = inputs(torch.float32, shape)
    e_dev, z_dev = nhwc(e, torch.float32), z.cuda()
    from afldm_amd import ops
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xg, Lg = x.cuda(), L.cuda()
    for _ in range(2):
        ops.hires_step(xg, e_dev, ref.cuda(), eps_ref.cuda(), z_dev, wt.cuda(), Lg, Lg, g, shape[1], coef, idx, advance=True, out=xg)
    assert int(idx.item()) == 2
    y = x
    for s in (0, 1):
        y, _ = launch(shape, y, e_dev, ref, eps_ref, z_dev, wt, L, s)
    assert torch.equal(xg.cpu(), y)


# ------------------------------------------------------------------------------------------------ afldm_hires_windows
def _fourier_shift(v, dy, dx):
    S = v.shape[-1]
    k = np.fft.fftfreq(S) * S
    return np.fft.ifft2(np.fft.fft2(v) * np.exp(2j * np.pi * (k[:, None] * dy + k[None, :] * dx) / S)).real


@pytest.mark.parametrize("shape", [GEOMS[1], GEOMS[2], GEOMS[3], GEOMS[4]])
def test_fully_filtered_dilated_views_are_fractional_shifts_of_one_another_on_the_device(shape):
    """f = 1: dilated view (i, j) is view (0, 0) shifted by (i / scale, j / scale).  Within the kernel's bound (1) + (3) plus what
    the same identity misses when evaluated in float64 with the fp32 matrix the kernel is given (printed): that matrix is the
    ideal low-pass only to its rounding, a property of the input and not of the kernel."""
    from afldm_amd import ops
    g, x, _, _, _, _, _, L = inputs(torch.float32, shape)
    scale = shape[1]
    wins = ops.hires_windows(x.cuda(), L.cuda(), L.cuda(), 1.0, g, scale).cpu()
    loc, dil = ho.split(wins, g, scale)
    assert torch.equal(loc, po.crop(x, g))
    want = ho.split(ho.hires_windows(x, L, 1.0, g, scale), g, scale)[1]
    t1 = 2e-6 * float(want.abs().max())
    t3 = 2.0 * float((ho.lowpass(x, L) - ho.lowpass(x, L, torch.float32)).abs().max())
    err = float((dil.double() - want).abs().max())

    def miss(v):
        v = v.double().numpy()
        return max(float(np.abs(v[P, i * scale + j, c] - _fourier_shift(v[P, 0, c], i / scale, j / scale)).max())
                   for P in range(v.shape[0]) for c in range(v.shape[2]) for i in range(scale) for j in range(scale))
    defect, got = miss(want), miss(dil)
    print(f"\n[shift identity {shape}] windows {err:.2e} of {t1 + t3:.2e} allowed; views against the shifts of view (0, 0): {got:.2e} of "
          f"{t1 + t3 + defect:.2e} allowed (kernel bound {t1 + t3:.2e} + the fp32 matrix's own defect {defect:.2e})")
    assert err <= t1 + t3 and got <= t1 + t3 + defect
    # f = 0 reads no matrix and gives the plain sub-lattices
    plain = ops.hires_windows(x.cuda(), None, None, 0.0, g, scale).cpu()
    assert torch.equal(ho.split(plain, g, scale)[1], ho.views(x, scale)) and torch.equal(ho.split(plain, g, scale)[0], loc)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_alone():
    from afldm_amd import _lib, ops
    from afldm_amd._lib import AfldmError
    from afldm_amd.panorama import Geometry
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")                # row 0: every term on
    P, C = 1, 2
    # buffers large enough for every geometry below, so that a refusal that came too late would still write inside them
    big = 80 * 80
    canvas, ref = torch.zeros(P * C * big, device="cuda"), torch.zeros(P * C * big, device="cuda")
    eps, noise = torch.zeros(64 * C * big, device="cuda"), torch.zeros(len(ROWS) * P * C * big, device="cuda")
    wt, L = torch.ones(big, device="cuda"), torch.zeros(big, device="cuda")
    out, wins = torch.full((P * C * big,), 3.0, device="cuda"), torch.full((64 * C * big,), 3.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 3.0).all()) and bool((wins == 3.0).all()) and int(idx.item()) == 0

    def step(Hc, Wc, S, oy, ox, scale, dtype_code=0, noise_stride=big * P * C):
        a, b = (ctypes.c_int * len(oy))(*oy), (ctypes.c_int * len(ox))(*ox)
        return _lib.lib.afldm_hires_step(canvas.data_ptr(), eps.data_ptr(), ref.data_ptr(), ref.data_ptr(), noise.data_ptr(), noise_stride,
                                         wt.data_ptr(), L.data_ptr(), L.data_ptr(), out.data_ptr(), wins.data_ptr(), coef.data_ptr(),
                                         idx.data_ptr(), 1, P, C, Hc, Wc, S, a, len(oy), b, len(ox), scale, dtype_code, stream)

    def windows(Hc, Wc, S, oy, ox, scale):
        a, b = (ctypes.c_int * len(oy))(*oy), (ctypes.c_int * len(ox))(*ox)
        return _lib.lib.afldm_hires_windows(canvas.data_ptr(), L.data_ptr(), L.data_ptr(), 0.5, wins.data_ptr(), P, C, Hc, Wc, S, a,
                                            len(oy), b, len(ox), scale, stream)
    ESHAPE = step(8, 10, 4, (0, 4), (0, 4), 2)
    assert ESHAPE != 0
    bad = [
        ((8, 10, 4, (0, 4), (0, 4, 6), 2), "square"),                     # Hc != Wc
        ((8, 8, 4, (0, 4), (0, 4), 3), "scale"),                          # Hc != scale S
        ((8, 8, 2, (0, 2, 4, 6), (0, 2, 4, 6), 2), "scale"),
        ((66, 66, 33, (0, 33), (0, 33), 2), "square"),                    # Hc > 64
        ((1, 1, 1, (0,), (0,), 1), "square"),                             # Hc < 2
        ((8, 8, 4, (0, 4), (0, 4), 0), "scale"),                          # scale < 1
        ((8, 8, 4, (0, 4), (0, 4), -2), "scale"),
        ((34, 34, 17, tuple(range(17)), (0, 17), 2), "origins"),          # more than 16 origins on an axis
        ((8, 8, 4, (0, 4), (0, 5), 2), "leaves"),                         # a window leaves the canvas
        ((8, 8, 4, (0, 4), (-1, 4), 2), "leaves"),
        ((12, 12, 4, (0, 4, 8), (0, 8), 3), "no window covers"),          # an uncovered coordinate
    ]
    for args, what in bad:
        assert step(*args) == ESHAPE, args
        assert what in _lib.lib.afldm_last_error().decode(), (args, _lib.lib.afldm_last_error())
        assert untouched(), args
        assert windows(*args) == ESHAPE, args
        assert untouched(), args
    assert step(8, 8, 4, (0, 4), (0, 4), 2, dtype_code=7) != 0 and untouched()             # an unknown dtype code
    assert step(8, 8, 4, (0, 4), (0, 4), 2, noise_stride=P * C * 64 - 1) != 0 and untouched()
    assert step(8, 8, 4, (0, 4), (0, 4), 2, noise_stride=P * C * 64) == 0                    # ... and with nothing wrong it goes through
    torch.cuda.synchronize()
    n, nw = P * C * 64, (4 + 4) * C * 16
    assert int(idx.item()) == 1 and not bool((out[:n] == 3.0).any()) and bool((out[n:] == 3.0).all())
    assert not bool((wins[:nw] == 3.0).any()) and bool((wins[nw:] == 3.0).all())             # ... and writes what it owns, no more
    # the binding's own checks
    g = Geometry.grid(8, 8, 4, 4, 4)
    c8, e8, L8, w4 = torch.zeros(1, 2, 8, 8, device="cuda"), torch.zeros(8, 4, 4, 2, device="cuda"), torch.eye(8, device="cuda"), \
        torch.ones(4, 4, device="cuda")
    ops.hires_step(c8, e8, c8, c8, None, w4, L8, L8, g, 2, coef, idx)
    with pytest.raises(ValueError):
        ops.hires_step(c8, e8[:7], c8, c8, None, w4, L8, L8, g, 2, coef, idx)                # a window short
    with pytest.raises(ValueError):
        ops.hires_step(c8, e8, c8[..., :7].contiguous(), c8, None, w4, L8, L8, g, 2, coef, idx)
    with pytest.raises(ValueError):
        ops.hires_step(c8, e8, c8, c8, None, w4, L8[:7, :7].contiguous(), L8, g, 2, coef, idx)
    with pytest.raises(ValueError):
        ops.hires_step(c8, e8, c8, c8, None, torch.ones(5, 5, device="cuda"), L8, L8, g, 2, coef, idx)
    with pytest.raises(ValueError):
        ops.hires_windows(c8, L8, L8, 0.5, Geometry.grid(8, 8, 4, 4, 4, circular_x=True), 2)
    with pytest.raises(AfldmError, match="scale"):
        ops.hires_windows(c8, L8, L8, 0.5, g, 4, out=torch.zeros(4 + 16, 2, 4, 4, device="cuda"))
