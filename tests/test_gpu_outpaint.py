"""The outpainting update on MI355X (csrc/pano.hip: afldm_pano_repaint_step, through ops.pano_repaint_step) against the float64
restatement of tests/outpaint_oracle.py on fp32-rounded coefficient rows, with eps in fp32 and bf16, hard, soft and broadcast
masks, a uniform and a random window weight.

Bound.  Not fixed in advance (tests/test_gpu_pano.py's construction):
  tol = 2e-6 M + 2 |u0| max(1 - m) (|a| err(mean x0) + |b| err(mean eps))
M is the maximum over the tensor of |want|, |u0 unknown| and |u0 knownp| - the blend can cancel, so the chain's roundings scale
with its parts, not with its result; 2e-6 is test_sde_step_kernel's figure for an fp32 chain of this length.  err(mean .) is
test_gpu_pano.mean_bound: the same weighted means taken in fp32 by torch on the CPU (ascending k, as the kernel) against float64.
Both terms and the kernel's error are printed.  What is exact is asserted with torch.equal: the windows are the crops of the
canvas, aliased and separate outputs, a canvas alone or second of two, one element per thread against four, kept elements on the
last row, unread noise slots full of NaN, where a NaN in eps arrives, and that a refusal writes nothing."""
import ctypes
import itertools
import math

import pytest
import torch

import outpaint_oracle as oo
import pano_oracle as po
from test_gpu_pano import GEOMS, f32, geometry, mean_bound, nhwc

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
INF = math.inf
# (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0)
ROWS = [
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.0, 0.8, 0.6, 1.0, 0.0, 0.0),      # DDIM-shaped: no clip, c = u1 = 0 (z_u, z_b not read)
    (1.0, -0.9, -1.0, 1.0, 0.55, 0.1, 0.2, 0.8, 0.6, 0.9, 0.43, 0.0),              # clipped, all three slots live
    (1 / 0.9, -0.3 / 0.9, -INF, INF, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0),      # the last evaluation: no slot read
]
LIVE = [(row[8] != 0.0, row[6] != 0.0, row[10] != 0.0) for row in ROWS]            # z_k, z_u, z_b
MASKS = ["hard", "soft", "one"]                                                    # "one": a batch-1 soft mask, broadcast by the caller


def inputs(dtype, shape, seed=29):
    """x, known, eps as NCHW fp32 holding what the kernel reads (eps rounded to dtype), three noise slots per ROWS entry, a
    non-uniform wt, and the masks [P, 1, Hc, Wc]."""
    P, C, S, Hc, Wc = shape[:5]
    g = geometry(shape)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, Hc, Wc, generator=gen)
    x[0, 0, 0, :4] = torch.tensor([0.5, -0.5, 0.75, -3.0])                 # on and beyond the clip of row 1
    e = torch.randn(P * g.nwin, C, S, S, generator=gen).to(dtype).float()
    known = torch.randn(P, C, Hc, Wc, generator=gen)
    z = torch.randn(len(ROWS), 3, P, C, Hc, Wc, generator=gen)
    wt = torch.rand(S, S, generator=gen) + 0.25
    hard = torch.zeros(P, 1, Hc, Wc)
    hard[..., Wc // 3: Wc // 3 + max(2, S // 2)] = 1.0                     # kept columns, some windows see both sides
    hard[0, 0, 0, 0] = 1.0                                                 # ... and the clip plants: one kept, three generated
    soft = torch.rand(P, 1, Hc, Wc, generator=gen) * 0.98 + 0.01           # in (0, 1)
    masks = {"hard": hard, "soft": soft, "one": soft[:1].expand(P, 1, Hc, Wc).contiguous()}
    return g, x, e, known, z, wt, masks


def poisoned(z):
    """NaN in every noise slot its coefficient row does not read: the kernel must not load it (0 * NaN is not 0)."""
    out = z.clone()
    for s, live in enumerate(LIVE):
        for j, on in enumerate(live):
            if not on:
                out[s, j] = math.nan
    return out


def step_bound(x, e, known, m, zs, wt, g, row, label):
    r = f32(row)
    want, wins, unknown, knownp = oo.outpaint_step(x, e, known, m, zs, wt, g, r)
    M = max(float(want.abs().max()), abs(r[9]) * float(unknown.abs().max()), abs(r[9]) * float(knownp.abs().max()))
    t1 = 2e-6 * M
    t2 = 2.0 * abs(r[9]) * float((1.0 - m.double()).max()) * (abs(r[4]) * mean_bound(po.x0_windows(x, e, g, r), wt, g)
                                                             + abs(r[5]) * mean_bound(e, wt, g))
    print(f"    {label}: bound terms (1) {t1:.2e} + (2) {t2:.2e}  (M {M:.2f})")
    return want, wins, t1 + t2


def launch(x, e_dev, known, m, z_dev, wt_dev, g, s, alias=True):
    from afldm_amd import ops
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    out, wins = ops.pano_repaint_step(xg, e_dev, known.cuda(), m.cuda(), z_dev, wt_dev, g, coef, idx, advance=False,
                                      out=xg if alias else None)
    assert (out.data_ptr() == xg.data_ptr()) == alias and int(idx.item()) == s
    if not alias:
        assert torch.equal(xg.cpu(), x)                                   # the input is left alone
    return out.cpu(), wins.cpu()


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, GEOMS)))
def test_pano_repaint_step_kernel(dtype, shape):
    g, x, e, known, z, wt, masks = inputs(dtype, shape)
    e_dev, ones, z_dev = nhwc(e, dtype), torch.ones(g.S, g.S), poisoned(z).cuda()
    print()
    cases = [(s, w, name) for s in range(len(ROWS)) for w, name in ((ones, "hard"), (ones, "soft"))]
    cases += [(1, wt, "soft"), (1, wt, "one"), (0, wt, "hard")]                                  # ... and a random wt > 0
    for s, w, name in cases:
        m = masks[name]
        label = f"{str(dtype)[6:]} {shape} row {s} {name} mask" + ("" if w is ones else " random wt")
        want, want_wins, tol = step_bound(x, e, known, m, z[s], w, g, ROWS[s], label)
        got, wins = launch(x, e_dev, known, m, z_dev, w.cuda(), g, s)
        assert torch.isfinite(got).all()
        err = float((got.double() - want).abs().max())
        print(f"        kernel max-abs error {err:.2e} of {tol:.2e} allowed")
        assert err <= tol, (s, name, err, tol)
        assert torch.equal(wins, po.crop(got, g))                         # the next UNet input is the canvas, cropped
        got2, wins2 = launch(x, e_dev, known, m, z_dev, w.cuda(), g, s, alias=False)
        assert torch.equal(got2, got) and torch.equal(wins2, wins)
        if name == "hard" and s == 2:                                     # the last evaluation returns kept elements bit for bit
            keep = (m == 1.0).expand_as(got)
            assert int(keep.sum()) > 0 and torch.equal(got[keep], known[keep])
        # the unread slots hold NaN; with zeros there instead the bits are the same
        got3, _ = launch(x, e_dev, known, m, z.cuda(), w.cuda(), g, s)
        assert torch.equal(got3, got)


@pytest.mark.parametrize("shape", [GEOMS[0], GEOMS[2], GEOMS[4]])
def test_canvas_bits_do_not_depend_on_the_batch(shape):
    """Every canvas of a batch of two, run alone (P = 1), gives the bits it gives inside the batch."""
    g, x, e, known, z, wt, masks = inputs(torch.float32, shape)
    assert x.shape[0] == 2
    n, m = g.nwin, masks["soft"]
    for s in range(len(ROWS)):
        both, wins = launch(x, nhwc(e, torch.float32), known, m, z.cuda(), wt.cuda(), g, s)
        for i in (0, 1):
            one, w1 = launch(x[i:i + 1], nhwc(e[i * n:(i + 1) * n], torch.float32), known[i:i + 1], m[i:i + 1],
                             z[:, :, i:i + 1].contiguous().cuda(), wt.cuda(), g, s)
            assert torch.equal(one, both[i:i + 1]) and torch.equal(w1, wins[i * n:(i + 1) * n]), (s, i)


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, [GEOMS[0], GEOMS[2], GEOMS[4]])))
def test_one_element_per_thread_and_four_give_the_same_bits(dtype, shape):
    """C = 4 with eps 16 bytes (fp32) or 8 bytes (bf16) aligned takes the four-channel path; the same eps in a view one element into
    a buffer is misaligned and takes the one-element path."""
    g, x, e, known, z, wt, masks = inputs(dtype, shape)
    assert shape[1] == 4
    wide = nhwc(e, dtype)
    buf = torch.empty(wide.numel() + 1, dtype=dtype, device="cuda")
    narrow = buf[1:].view(wide.shape)
    narrow.copy_(wide)
    assert wide.data_ptr() % 16 == 0 and narrow.data_ptr() % (4 * wide.element_size()) != 0 and narrow.is_contiguous()
    for s in range(len(ROWS)):
        a, wa = launch(x, wide, known, masks["soft"], z.cuda(), wt.cuda(), g, s)
        b, wb = launch(x, narrow, known, masks["soft"], z.cuda(), wt.cuda(), g, s)
        assert torch.equal(a, b) and torch.equal(wa, wb), s


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, [GEOMS[1], GEOMS[2], GEOMS[4]])))
def test_a_nan_in_eps_reaches_what_its_window_covers_where_the_mask_lets_it(dtype, shape):
    P, C, S = shape[:3]
    g, x, e, known, z, wt, masks = inputs(dtype, shape)
    k = g.nwin - 1                                                       # the last window of the last canvas
    oy, ox = g.corners()[k]
    rows, cols = [(oy + u) % g.Hc for u in range(S)], [(ox + v) % g.Wc for v in range(S)]
    m = masks["soft"].clone()
    m[P - 1, 0, rows[1], cols[0]:cols[0] + 1] = 1.0                       # kept elements inside the window ...
    m[P - 1, 0, rows[0], cols[S - 1]] = 1.0
    m[P - 1, 0, rows[2], cols[1]] = 0.0                                   # ... and a fully generated one
    clean, clean_wins = launch(x, nhwc(e, dtype), known, m, z.cuda(), wt.cuda(), g, 1)
    bad = e.clone()
    bad[(P - 1) * g.nwin + k] = math.nan
    got, wins = launch(x, nhwc(bad, dtype), known, m, z.cuda(), wt.cuda(), g, 1)
    where = torch.zeros_like(got, dtype=torch.bool)
    where[P - 1][:, torch.tensor(rows)[:, None], torch.tensor(cols)[None, :]] = True
    where &= (m < 1.0).expand_as(where)
    assert int(where.sum()) == C * (S * S - 2)
    assert torch.equal(torch.isnan(got), where)
    assert torch.equal(torch.isnan(wins), po.crop(where, g))
    assert torch.equal(got.nan_to_num(7.0), torch.where(where, torch.full_like(got, 7.0), clean))
    # one element of one channel: that canvas element and its crops, nothing else
    ch, u, v = C - 1, 1, S - 1
    bad = e.clone()
    bad[(P - 1) * g.nwin + k, ch, u, v] = math.nan
    got, wins = launch(x, nhwc(bad, dtype), known, m, z.cuda(), wt.cuda(), g, 1)
    where = torch.zeros_like(got, dtype=torch.bool)
    where[P - 1, ch, rows[u], cols[v]] = True
    assert torch.equal(torch.isnan(got), where) and torch.equal(torch.isnan(wins), po.crop(where, g))
    assert int(torch.isnan(wins).sum()) >= 1


def test_pano_repaint_step_advances_like_the_other_updates():
    from afldm_amd import ops
    g, x, e, known, z, wt, masks = inputs(torch.float32, GEOMS[0])
    e_dev, z_dev, w_dev, m = nhwc(e, torch.float32), z.cuda(), wt.cuda(), masks["soft"]
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    for _ in range(2):
        ops.pano_repaint_step(xg, e_dev, known.cuda(), m.cuda(), z_dev, w_dev, g, coef, idx, advance=True, out=xg)
    assert int(idx.item()) == 2
    y = x
    for s in (0, 1):
        y, _ = launch(y, e_dev, known, m, z_dev, w_dev, g, s)
    assert torch.equal(xg.cpu(), y)


def test_refusals_leave_the_outputs_alone():
    from afldm_amd import _lib, ops
    from afldm_amd._lib import AfldmError
    from afldm_amd.panorama import Geometry
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    idx = torch.ones(1, dtype=torch.int32, device="cuda")                 # row 1: every coefficient live
    P, C = 1, 4

    def buffers(g):
        canvas = torch.zeros(P, C, g.Hc, g.Wc, device="cuda")
        eps = torch.zeros(P * g.nwin, g.S, g.S, C, device="cuda")
        mask = torch.zeros(P, 1, g.Hc, g.Wc, device="cuda")
        noise = torch.zeros(len(ROWS), 3, P, C, g.Hc, g.Wc, device="cuda")
        out, wins = torch.full_like(canvas, 3.0), torch.full((P * g.nwin, C, g.S, g.S), 3.0, device="cuda")
        return canvas, eps, mask, noise, torch.ones(g.S, g.S, device="cuda"), out, wins

    def untouched(out, wins):
        torch.cuda.synchronize()
        return bool((out == 3.0).all()) and bool((wins == 3.0).all()) and int(idx.item()) == 1
    bad = [
        (Geometry(4, 11, 4, (0,), (0, 7)), "no window covers"),
        (Geometry(4, 11, 4, (0,), (0, 4, 8)), "leaves"),
        (Geometry(4, 9, 4, (0,), (0, 3, 9), False, True), "leaves"),
        (Geometry(4, 34, 4, (0,), tuple(range(0, 32, 2)) + (30,)), "origins"),
        (Geometry(4, 3, 4, (0,), (0,)), "canvas"),
    ]
    for g, what in bad:
        canvas, eps, mask, noise, ones, out, wins = buffers(g)
        with pytest.raises(AfldmError, match=what):
            ops.pano_repaint_step(canvas, eps, canvas, mask, noise, ones, g, coef, idx, advance=True, out=out, windows_out=wins)
        assert untouched(out, wins)
    # the C entry point itself: NULL noise under a row whose coefficients are live, strides shorter than a slot or than three
    # slots, an unknown dtype code
    g = geometry(GEOMS[0])
    canvas, eps, mask, noise, ones, out, wins = buffers(g)
    n = canvas.numel()

    def call(noise_ptr, step_stride, slot_stride, dtype_code):
        oy, ox = (ctypes.c_int * g.ny)(*g.oy), (ctypes.c_int * g.nx)(*g.ox)
        return _lib.lib.afldm_pano_repaint_step(canvas.data_ptr(), eps.data_ptr(), canvas.data_ptr(), mask.data_ptr(), noise_ptr,
                                                step_stride, slot_stride, ones.data_ptr(), out.data_ptr(), wins.data_ptr(),
                                                coef.data_ptr(), idx.data_ptr(), 1, P, C, g.Hc, g.Wc, g.S, oy, g.ny, ox, g.nx, 0, 0,
                                                dtype_code, torch.cuda.current_stream().cuda_stream)
    for args in ((None, 3 * n, n, 0), (noise.data_ptr(), 3 * n, n - 1, 0), (noise.data_ptr(), 3 * n - 1, n, 0),
                 (noise.data_ptr(), 3 * n, n, 7)):
        assert call(*args) != 0, args
        assert untouched(out, wins), args
    assert call(noise.data_ptr(), 3 * n, n, 0) == 0                        # ... and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert int(idx.item()) == 2 and not bool((out == 3.0).any())
    # the binding's own checks
    with pytest.raises(ValueError):
        ops.pano_repaint_step(canvas, eps, canvas, mask[..., :-1].contiguous(), noise, ones, g, coef, idx)
    with pytest.raises(ValueError):
        ops.pano_repaint_step(canvas, eps, canvas[..., :-1].contiguous(), mask, noise, ones, g, coef, idx)
    with pytest.raises(ValueError):
        ops.pano_repaint_step(canvas, eps, canvas, mask, noise, torch.ones(5, 5, device="cuda"), g, coef, idx)
