"""Case lists, float64 references and comparisons for the plumbing launches (csrc/misc.hip: layout, cast, timestep
embedding, SiLU, step prologue, masked metrics, DDIM) and for afldm_upfirdn2d (csrc/fir.hip).  Plain torch / numpy on
the CPU; tests/test_plumbing_oracle_host.py proves that the references and the comparisons catch planted faults,
tests/test_gpu_plumbing.py and tests/test_gpu_fir_edges.py hold the kernels to them.

Addressed values.  Element i of a tensor holds a value that names i: i itself in fp32 (exact below 2^24, every size
here is), and in bf16 the integer (i mod 251) - 125, which bf16 holds exactly (|v| <= 125 < 2^8).  Two bf16 elements
share a value exactly when their indices differ by a multiple of 251 (a prime): neighbours, and every displacement
d with d % 251 != 0, stay distinct.  `addressed_strides_ok` states that for the strides a layout case moves elements
by; the fp32 form has no such period and runs the same index arithmetic (the kernels are templates over the dtype).

Exact FIR inputs.  x holds integers in [-8, 8], 2-D taps are multiples of 1/8 in [-2, 2], 1-D taps multiples of 1/4
in [-1.25, 1.25] (their outer product: multiples of 1/16 in [-1.5625, 1.5625]), gains are powers of two.  Every
partial sum is then a multiple of q = tap quantum x gain quantum with magnitude at most sum|tap| x 8 x gain;
`fir_exact` checks sum|tap| x 8 x gain / q < 2^24 for a case, so that any summation order gives the same fp32 value
and the float64 reference is that value.

Tolerances (u = 2^-24, the relative error of one fp32 rounding; "1 ulp" of a function = 2u relative at worst).
ROCm ships no accuracy table for the device math library, so the classes are the ones the device library's source
states for fp32: expf 1 ulp, sinf 1 ulp, cosf 1 ulp; the hardware exp2 / reciprocal are of the 1 ulp class
(csrc/common.hpp).

  timestep embedding (k_timestep_embedding): e = (C * k) / (half - shift), w = expf(e), a = t * w, out = sin/cos(a).
    * C = fp32(-ln 10000) differs from -ln 10000 by 0.24u relative (EMB_CONST_ERR, computed below); C * k rounds
      once (1u), the divisor is exact (small integers), the quotient rounds once (1u): e carries 2.24u relative,
      that is 2.24u |e| absolute, which expf turns into 2.24u |e| relative in w.
    * expf: 2u.  t * w: 1u.  So |a_fp32 - a| <= u |a| (2.24 |e| + 3), and sin / cos move by at most that.
    * |e| = ln(t / |a|) <= ln(T / |a|) with T = 999, the largest timestep: g(a) = a (2.24 ln(T / a) + 3) is concave
      in a, so its tangent at any a0 bounds it from above on (0, T].  At a0 = 600 the tangent is
      c2 = 2.24 ln(999/600) + 3 - 2.24 = 1.902 -> 1.91 and an intercept of 2.24 * 600 = 1344.
    * sinf / cosf: 1 ulp of a result of magnitude <= 1: 2u.   c1 = 1344 + 2 = 1346 -> EMB_C1 = 1346, EMB_C2 = 1.91.
    * At |a| = 10^3 the bound is u (1346 + 1910) = 1.94e-4 <= the 2e-4 the first test of this kernel allows
      everywhere, and it falls to 8.0e-5 at a = 0.
  SiLU (silu_f): m = x * K, E = exp2(m), r = rcp(1 + E), y = x * r with K = fp32(-log2 e).
    * K is 0.22u off (SILU_CONST_ERR), the product rounds once: m carries 1.22u relative, so E carries
      ln 2 * |m| * 1.22u = 1.22u |x| <= 1.5u |x| relative; the hardware exp2 adds 2u.  Both reach y through
      E / (1 + E) = sigmoid(-x) <= 1.
    * 1 + E rounds once (1u), the reciprocal is 2u, the final product 1u: 4u.
    * tol = u |ref| (4 + (2 + 1.5 |x|) sigmoid(-x)) + 2^-126, never above the form u |ref| (c + 1.5 |x|) with
      c = SILU_C = 6; the last term is one denormal threshold for results the hardware flushes.  On |x| <= 4 it stays
      below the 1e-6 the first test of this kernel allows (9.7e-7 at x = 4; the host test checks the grid).
  DDIM: rtol = atol-scale = 2e-6, the bound tests/test_gpu_sde.py::test_sde_step_kernel uses for an fp32 elementwise
    chain, the scale being the largest magnitude among x, sa_p x0 and sb_p eps.
  Real-valued FIR: u (fh fw + 2) sum|tap x| per element (one rounding per fused multiply-add, the gain product and
    slack for the reference's own fp32 taps), plus 2^-8 |ref| for a bf16 store.
"""
import collections
import math

import numpy as np
import torch

U = 2.0 ** -24
DENORM = 2.0 ** -126
GRID_REACH = 2048 * 256                 # elements one pass of an elementwise grid covers (misc.hip ew_grid)
FIR_GRID_PLANES = 4096                  # fir.hip: planes beyond this run the plane loop
FIR_COPY_TAPS = 256                     # fir.hip: taps beyond this run a second pass of the tap copy
FIR_MAX_TAP_BYTES = 64 * 1024
DTYPES = (torch.float32, torch.bfloat16)

EMB_CONST_ERR = abs(float(np.float32(-9.210340371976184)) + math.log(10000.0)) / math.log(10000.0) / U
SILU_CONST_ERR = abs(float(np.float32(-1.4426950408889634)) + 1 / math.log(2.0)) * math.log(2.0) / U
EMB_T_MAX = 999.0
EMB_E_REL = 2.24                        # >= EMB_CONST_ERR + 2 (host test)
EMB_C1, EMB_C2 = 1346.0, 1.91
SILU_C = 6.0


# ------------------------------------------------------------------------------------------------ addressed values
def addressed(n, dtype):
    i = torch.arange(n, dtype=torch.int64)
    if dtype == torch.float32:
        assert n < 2 ** 24
        return i.to(torch.float32)
    return ((i % 251) - 125).to(torch.float32).to(torch.bfloat16)


def addressed_strides_ok(strides):
    return all(int(s) % 251 != 0 for s in strides if int(s) != 0)


def bits(t):
    """Bit patterns of an fp32 / bf16 tensor as integers."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_identical(got, want, what="", by_bits=False, names=None, extra=""):
    """got must equal want element for element (NaN matches NaN; with by_bits the bit patterns must match, so -0 is not
    +0).  A failure names the first differing element: its flat and unravelled index, what it holds and what it should
    hold - on addressed fp32 data those two values are the source indices fetched and wanted."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = torch.isnan(got), torch.isnan(want)
    if by_bits:
        bad = (bits(got) != bits(want)) & ~(gn & wn)
    else:
        bad = ((got != want) & ~(gn & wn)) | (gn != wn)
    if bool(bad.any()):
        flat = int(torch.nonzero(bad.reshape(-1))[0])
        idx = np.unravel_index(flat, tuple(got.shape)) if got.ndim else ()
        where = ", ".join(f"{n}={int(v)}" for n, v in zip(names, idx)) if names else str(tuple(int(v) for v in idx))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first at flat {flat} ({where}): "
                             f"got {float(got.reshape(-1)[flat])!r}, want {float(want.reshape(-1)[flat])!r} {extra}")


def worst_over_bound(got, ref, tol):
    """(max of |got - ref| / tol, flat index of it); a non-finite got where ref is finite counts as infinite."""
    got, ref, tol = got.double().reshape(-1), ref.double().reshape(-1), tol.double().reshape(-1)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got) | ~torch.isfinite(ref), err, torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    k = int(ratio.nan_to_num(nan=math.inf).argmax())
    return float(ratio.nan_to_num(nan=math.inf)[k]), k


def assert_within(got, ref, tol, what):
    worst, k = worst_over_bound(got, ref, tol)
    over = int(((got.double() - ref.double()).abs().reshape(-1) > tol.double().reshape(-1)).sum())
    print(f"{what}: worst error / bound = {worst:.3f} at element {k}; {over} of {ref.numel()} elements over the bound")
    assert worst <= 1.0, (what, worst, k, float(got.reshape(-1)[k]), float(ref.reshape(-1)[k]), float(tol.reshape(-1)[k]))
    return worst


# ------------------------------------------------------------------------------------------------ rounding probes
def rounding_probes():
    """fp32 values whose bf16 rounding decides something: exact ties above an even and above an odd bf16 mantissa (RNE
    goes down / up), just off the ties, the largest finite fp32 (rounds to +inf), the largest finite bf16, signed zeros,
    denormals (a bf16 denormal, an fp32-only one, the smallest), infinities and NaN."""
    def f(b):
        return np.array([b], dtype=np.uint32).view(np.float32)[0]
    v = [f(0x3F808000), f(0x3F818000), f(0x3F808001), f(0x3F807FFF), f(0x3F817FFF), f(0xBF808000), f(0xBF818000),
         f(0x7F7FFFFF), f(0xFF7FFFFF), f(0x7F7F0000), f(0x7F7F8000), f(0x7F7F7FFF),
         0.0, f(0x80000000), f(0x00400000), f(0x00008000), f(0x00018000), f(0x00000001), f(0x80000001), f(0x007FFFFF),
         math.inf, -math.inf, math.nan, 1.0, -2.5, 3.0, 255.0, 257.0, 1e-30, -1e30]
    return torch.tensor(np.array(v, dtype=np.float32))


def expected_bf16(x32):
    """The RNE rounding of fp32 values, as torch does it (compared as int16 bit patterns, NaN as NaN-ness)."""
    return x32.to(torch.bfloat16)


def truncate_bf16(x32):
    """bf16 by dropping the low 16 bits: the planted rounding fault."""
    b = x32.contiguous().view(torch.int32)
    return (b & -65536).view(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ layout
LAYOUT_SHAPES = [                       # (B, C, H, W) of to_nhwc / to_nchw
    (2, 1, 3, 5), (3, 4, 1, 1), (2, 3, 5, 7), (1, 8, 4, 6), (1, 192, 3, 3), (2, 5, 1, 9),
    (1, 4, 256, 512),                   # 524 288 elements: exactly the grid's reach
    (1, 3, 1, 349527),                  # 2 x 524 288 + 5 elements, C and HW both odd: three passes of the grid-stride loop
]
PACK_SHAPES = [                         # (O, I, KH, KW), or (O, I) for a linear weight
    (3, 1, 1, 1), (5, 3, 3, 3), (2, 4, 1, 3), (3, 8, 2, 2), (1, 192, 3, 3), (7, 5), (1, 1),
    (64, 128, 8, 8),                    # 524 288
    (3, 349527, 1, 1),                  # 2 x 524 288 + 5
    (349527, 1, 3, 1),                  # the same count with I = 1 and a non-square kernel
]
CAST_SIZES = [1, 255, 257, 2 * GRID_REACH + 5]


def nhwc_reference(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw_reference(y):
    return y.permute(0, 3, 1, 2).contiguous()


def pack_reference(w):
    return (w[:, :, None, None] if w.ndim == 2 else w).permute(0, 2, 3, 1).contiguous()


def with_canaries(shape, dtype, device, guard=64, canary=-77.0):
    """(buffer, view): a contiguous view of `shape` inside a buffer that holds `canary` on both sides of it (the guard is
    a multiple of 16 bytes, so the view keeps the buffer's alignment)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), canary, dtype=dtype, device=device)
    return buf, buf[guard:guard + n].view(shape)


def canaries_intact(buf, n, guard=64, canary=-77.0):
    b = buf.float().cpu()
    return bool((b[:guard] == canary).all()) and bool((b[guard + n:] == canary).all())


# ------------------------------------------------------------------------------------------------ step prologue
ROW_BYTES = [16, 16 * 1024, 16 * 1024 + 16]          # 1, 1024 and 1025 chunks: the copy loop's second pass
STEP_ROWS = 5


def step_table(row_bytes, dtype, rows=STEP_ROWS):
    """(tvals [rows] fp32, table [rows, row elements]) of addressed rows."""
    per = row_bytes // (4 if dtype == torch.float32 else 2)
    table = addressed(rows * per, dtype).reshape(rows, per)
    tvals = torch.tensor([900.0 - 7.0 * r for r in range(rows)], dtype=torch.float32)
    return tvals, table


def step_row_reference(tvals, table, step, pre_advance):
    """(row, t, step afterwards) of afldm_select_step_row / afldm_select_timestep."""
    s = step + 1 if pre_advance else step
    return (None if table is None else table[s].clone()), tvals[s].clone(), s


# ------------------------------------------------------------------------------------------------ masked metrics
METRIC_SIZES = [1, 63, 255, 256, 257, 4099]


def metrics_case(n, dtype, seed=0, B=3):
    """a, b integer-valued in [-8, 8], 0/1 masks, per sample: sample 0 under a random mask, sample 1 fully masked out,
    sample 2 all negative under a partial mask (its maximum is the 0 of a masked-out element).  For n = 1 sample 2 is
    masked out as well, so that its maximum is 0 too."""
    g = torch.Generator().manual_seed(1000 + seed + n)
    a = torch.randint(-8, 9, (B, n), generator=g).float()
    b = torch.randint(-8, 9, (B, n), generator=g).float()
    m = (torch.rand(B, n, generator=g) > 0.4).float()
    m[1] = 0
    a[2] = -1 - a[2].abs()
    b[2] = -1 - b[2].abs()
    m[2, 0] = 0
    if n > 1:
        m[2, 1] = 1
    return a.to(dtype), b.to(dtype), m


def metrics_reference(a, b, m):
    """float64 [B, 6]: sum ((a - b) m)^2, sum m, max a m, min a m, max b m, min b m over each sample (a * m as the
    reference writes it: a masked-out element contributes 0 to the extrema)."""
    B = a.shape[0]
    m = m.double().expand_as(a).reshape(B, -1)
    a, b = a.double().reshape(B, -1), b.double().reshape(B, -1)
    am, bm = a * m, b * m
    return torch.stack([((am - bm) ** 2).sum(1), m.sum(1), am.max(1).values, am.min(1).values, bm.max(1).values,
                        bm.min(1).values], dim=1)


# ------------------------------------------------------------------------------------------------ timestep embedding
EMB_WIDTHS = [2, 6, 192, 896]


def emb_timesteps():
    return torch.cat([torch.arange(1000, dtype=torch.float32), torch.tensor([0.5, 998.75])])


def emb_reference(t32, dim, flip=True, freq_shift=0.0):
    """(out float64 [rows, dim], |a| float64 [rows, dim]) with the exponent, the frequency, the product and sin / cos in
    float64 on the fp32 timestep."""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    a = t32.double()[:, None] * torch.exp(-math.log(10000.0) * k / (half - float(freq_shift)))[None]
    s, c = torch.sin(a), torch.cos(a)
    out = torch.cat([c, s], 1) if flip else torch.cat([s, c], 1)
    return out, torch.cat([a, a], 1).abs()


def emb_tolerance(a_abs):
    return U * (EMB_C1 + EMB_C2 * a_abs)


def emb_error_bound(a_abs, t_max=EMB_T_MAX):
    """The counted bound itself, u (|a| (2.24 ln(T / |a|) + 3) + 2): emb_tolerance must dominate it (host test)."""
    a = a_abs.clamp_min(1e-300)
    return U * (a * (EMB_E_REL * torch.log(t_max / a).clamp_min(0) + 3) + 2)


# ------------------------------------------------------------------------------------------------ SiLU
def silu_points():
    grid = torch.linspace(-100.0, 100.0, 4096, dtype=torch.float64).float()
    extra = torch.tensor([2.0 ** -130, -2.0 ** -130, 1e-30, -1e-30, 88.0, -88.0], dtype=torch.float32)
    return torch.cat([grid, extra])


def silu_reference(x):
    x = x.double()
    return x / (1 + torch.exp(-x))


def silu_tolerance(x, ref):
    x = x.double()
    return U * ref.abs() * (4 + (2 + 1.5 * x.abs()) * torch.sigmoid(-x)) + DENORM


# ------------------------------------------------------------------------------------------------ DDIM
DDIM_SHAPES = [(3, 4, 8, 8), (2, 3, 5, 5), (1, 4, 1, 1), (1, 5, 363, 363)]
DDIM_ROWS = [(7.0, 11.0, 13.0, 17.0),                        # sentinel: a launch that reads row 0 is far off
             (0.8, 0.6, 0.9, 0.43588989435406733),           # the row in use (step_idx = 1)
             (-3.0, 19.0, 23.0, -29.0)]                      # sentinel
DDIM_GATHER_ROW = (1.0, 0.0, 0.0, 1.0)                       # x_prev = eps exactly when x = 0
DDIM_TOL = 2e-6


def ddim_reference(x, eps, row32):
    """float64 update from the fp32 coefficient row and the eps values the kernel reads (NCHW, already rounded);
    returns (x_prev, the scale of the tolerance)."""
    sa_t, sb_t, sa_p, sb_p = (float(v) for v in torch.tensor(row32, dtype=torch.float32))
    x, e = x.double(), eps.double()
    x0 = (x - sb_t * e) / sa_t
    scale = max(float(x.abs().max()), float((sa_p * x0).abs().max()), float((sb_p * e).abs().max()))
    return sa_p * x0 + sb_p * e, scale


def ddim_tolerance(ref, scale):
    return DDIM_TOL * ref.abs() + DDIM_TOL * scale


# ------------------------------------------------------------------------------------------------ FIR
FirRoute = collections.namedtuple("FirRoute", "route last_group RY x_blocks plane_loop tap_loop")


def fir_case(name, planes, H, W, fh, fw, up=(1, 1), down=(1, 1), pad=(0, 0, 0, 0), flip=False, gain=1.0, offset=False,
             f1d=False):
    """planes = (B, C); up / down = (x, y); pad = (x0, x1, y0, y1); offset: the input's storage starts one element past
    a 16-byte boundary; f1d: the filter is 1-D with fh = fw taps (the 2-D launch gets its outer product)."""
    assert not f1d or fh == fw
    return dict(name=name, planes=planes, H=H, W=W, fh=fh, fw=fw, up=up, down=down, pad=pad, flip=flip, gain=gain,
                offset=offset, f1d=f1d)


def fir_out_size(c):
    upW = c["W"] * c["up"][0] + c["pad"][0] + c["pad"][1]
    upH = c["H"] * c["up"][1] + c["pad"][2] + c["pad"][3]
    assert upW >= c["fw"] and upH >= c["fh"], c["name"]
    return (upH - c["fh"]) // c["down"][1] + 1, (upW - c["fw"]) // c["down"][0] + 1


def fir_route(c):
    """The choices launch_upfirdn2d and k_upfirdn2d make for a case (fir.hip): the column route of the launch (`vec`:
    one vector load per tap, needs fw = 1, no x re-sampling, padx0 = 0, W % 4 = 0 and an input aligned to four elements;
    `slide`: the register window, no x re-sampling; `general` otherwise), the route of its last column group (a vec
    thread whose four columns run past W slides), the row template RY (4 from 16 output rows on), the number of x
    blocks of 256 columns, whether the plane loop and the tap copy loop run a second pass."""
    outH, outW = fir_out_size(c)
    slide = c["up"][0] == 1 and c["down"][0] == 1
    vec = slide and c["fw"] == 1 and c["pad"][0] == 0 and c["W"] % 4 == 0 and not c["offset"]
    route = "vec" if vec else "slide" if slide else "general"
    last = route
    if vec and 4 * ((outW - 1) // 4) + 4 > c["W"]:
        last = "slide"
    return FirRoute(route, last, 4 if outH >= 16 else 1, (outW + 255) // 256, c["planes"][0] * c["planes"][1] > FIR_GRID_PLANES,
                    c["fh"] * c["fw"] > FIR_COPY_TAPS)


def _fir_cases():
    L = []
    col = dict(fh=3, fw=1, pad=(0, 0, 1, 1))                                  # a pure column filter: the vec conditions
    L.append(fir_case("vec", (2, 3), 6, 12, **col))
    L.append(fir_case("vec_w_odd", (2, 3), 6, 13, **col))                     # W % 4 != 0: slides
    L.append(fir_case("vec_padx1", (2, 3), 6, 12, fh=3, fw=1, pad=(0, 3, 1, 1)))   # mixed launch
    L.append(fir_case("vec_crop_x1", (1, 2), 6, 12, fh=3, fw=1, pad=(0, -2, 1, 0)))
    L.append(fir_case("vec_offset", (2, 3), 6, 12, offset=True, **col))       # misaligned storage: slides
    for fw in (2, 7):
        for px0 in (-1, 0, 2):
            L.append(fir_case(f"slide_fw{fw}_padx0_{px0}", (1, 3), 7, 21, fh=2, fw=fw, pad=(px0, fw, 1, 0),
                              flip=px0 == 0, gain=(1.0, 0.5, 4.0)[px0 % 3]))
    L.append(fir_case("slide_fw_gt_W", (1, 2), 5, 3, fh=1, fw=7, pad=(3, 3, 0, 0)))
    L.append(fir_case("slide_1d", (2, 2), 9, 11, fh=7, fw=7, pad=(3, 3, 3, 3), gain=4.0, f1d=True))
    ratios = [(2, 1), (1, 2), (3, 2)]
    for i, (ux, dx) in enumerate(ratios):
        uy, dy = ratios[(i + 1) % 3]                                          # the y ratio is another one
        L.append(fir_case(f"general_x{ux}{dx}_y{uy}{dy}", (1, 3), 9, 11, fh=4, fw=5, up=(ux, uy), down=(dx, dy),
                          pad=(2, 1, 1, 2), flip=bool(i & 1), gain=(1.0, 0.5, 4.0)[i]))
    for side in range(4):                                                    # a crop on each side
        pad = [2, 2, 2, 2]
        pad[side] = -2
        L.append(fir_case(f"general_crop{side}", (1, 2), 8, 10, fh=3, fw=3, up=(2, 2), down=(1, 1), pad=tuple(pad),
                          flip=bool(side & 1)))
    L.append(fir_case("general_1d", (1, 3), 7, 9, fh=5, fw=5, up=(3, 3), down=(2, 2), pad=(2, 2, 2, 2), f1d=True))
    for outW in (255, 256, 257, 513):                                        # a second and a third x block
        H = 17 if outW in (255, 513) else 5                                  # ... on both row templates (257: RY 1, 513: RY 4)
        Wv = (outW // 4) * 4
        L.append(fir_case(f"vec_w{outW}", (1, 2), H, Wv, fh=3, fw=1, pad=(0, outW - Wv, 1, 1)))
        L.append(fir_case(f"slide_w{outW}", (1, 2), H, outW, fh=2, fw=3, pad=(1, 1, 1, 0)))
        Wg = (outW + 1) // 2                                                 # up 2, 4 taps: outW = 2 Wg + padx0 + padx1 - 3
        L.append(fir_case(f"general_w{outW}", (1, 2), H, Wg, fh=2, fw=4, up=(2, 1), pad=(2, outW + 1 - 2 * Wg, 1, 0)))
    for outH in (1, 15, 16, 17):                                             # both templates, a partial last row group
        L.append(fir_case(f"slide_h{outH}", (1, 3), outH, 9, fh=3, fw=2, pad=(1, 0, 1, 1)))
    L.append(fir_case("general_h18", (1, 2), 9, 9, fh=3, fw=3, up=(2, 2), pad=(1, 1, 1, 1)))
    L.append(fir_case("planes_4097", (4097, 1), 4, 4, fh=1, fw=1))
    L.append(fir_case("taps_17x16", (1, 2), 20, 20, fh=17, fw=16, flip=True))
    L.append(fir_case("taps_128x128", (1, 1), 128, 128, fh=128, fw=128, pad=(1, 0, 1, 1)))
    return L


FIR_CASES = _fir_cases()
FIR_REFUSED = dict(planes=1, H=130, W=130, fh=129, fw=128)                   # one tap row past the 64 KiB buffer


def fir_inputs(c, seed=None):
    """(x fp32 [B, C, H, W] of integers in [-8, 8], f fp32: [fh, fw] multiples of 1/8 in [-2, 2], or [taps] multiples of
    1/4 in [-1.25, 1.25] for a 1-D case)."""
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])) if seed is None else seed)
    x = torch.randint(-8, 9, (*c["planes"], c["H"], c["W"]), generator=g).float()
    if c["f1d"]:
        f = torch.randint(-5, 6, (c["fw"],), generator=g).float() / 4
    else:
        f = torch.randint(-16, 17, (c["fh"], c["fw"]), generator=g).float() / 8
    f.view(-1)[0] = 0.5                                                       # never an all-zero filter; asymmetric ends
    f.view(-1)[-1] = -0.25
    return x, f


def fir_filter_2d(c, f):
    return torch.outer(f, f) if c["f1d"] else f


def fir_exact(c, f):
    """True if every partial sum of the case is exact in fp32 in any order (module docstring)."""
    f2 = fir_filter_2d(c, f).double() * c["gain"]
    q = (1 / 16 if c["f1d"] else 1 / 8) * min(c["gain"], 1.0)
    return bool(((f2 / q) == (f2 / q).round()).all()) and float(f2.abs().sum()) * 8 / q < 2 ** 24


def fir_kwargs(c):
    return dict(up=list(c["up"]), down=list(c["down"]), padding=list(c["pad"]), flip_filter=c["flip"], gain=c["gain"])


def fir_reference(c, x, f):
    """oracle.upfirdn.upfirdn2d on a float64 x (the taps stay fp32, as the oracle asks)."""
    from oracle import upfirdn as ou
    return ou.upfirdn2d(x.double(), f, **fir_kwargs(c))


def fir_reference_two_pass(c, x, f, dtype):
    """What the separable route of af_libs.torch_utils.ops.upfirdn2d computes for a 1-D filter: a row pass and a column
    pass, each with sqrt(gain), the intermediate stored in `dtype`."""
    from oracle import upfirdn as ou
    g = c["gain"] ** 0.5
    px0, px1, py0, py1 = c["pad"]
    y = ou.upfirdn2d(x.double(), f[None, :].contiguous(), up=[c["up"][0], 1], down=[c["down"][0], 1], padding=[px0, px1, 0, 0],
                     flip_filter=c["flip"], gain=g)
    y = y.to(dtype).double()
    return ou.upfirdn2d(y, f[:, None].contiguous(), up=[1, c["up"][1]], down=[1, c["down"][1]], padding=[0, 0, py0, py1],
                        flip_filter=c["flip"], gain=g)


def fir_loop(c, x, f2, drop_tap_row=None, flip=None):
    """The operator spelt out in float64 numpy: zero-stuff, pad / crop, correlate with the (flipped unless flip_filter)
    taps times the gain, decimate.  drop_tap_row / flip plant faults."""
    x = x.double().numpy()
    f2 = f2.double().numpy() * c["gain"]
    flip = c["flip"] if flip is None else flip
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = c["up"], c["down"], c["pad"]
    B, C, H, W = x.shape
    z = np.zeros((B, C, H * uy, W * ux))
    z[:, :, ::uy, ::ux] = x
    z = np.pad(z, ((0, 0), (0, 0), (max(py0, 0), max(py1, 0)), (max(px0, 0), max(px1, 0))))
    z = z[:, :, max(-py0, 0):z.shape[2] - max(-py1, 0), max(-px0, 0):z.shape[3] - max(-px1, 0)]
    taps = f2 if flip else f2[::-1, ::-1]                  # correlation taps
    fh, fw = taps.shape
    oh, ow = z.shape[2] - fh + 1, z.shape[3] - fw + 1
    out = np.zeros((B, C, oh, ow))
    for fy in range(fh):
        if fy == drop_tap_row:
            continue
        for fx in range(fw):
            out += taps[fy, fx] * z[:, :, fy:fy + oh, fx:fx + ow]
    return torch.from_numpy(np.ascontiguousarray(out[:, :, ::dy, ::dx]))


def fir_names():
    return ("b", "c", "oy", "ox")


def real_fir_case():
    """One case with real-valued data: a 13-tap Lanczos-like 1-D filter at a fractional offset on a 3 x 37 x 261 input."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(1, 3, 37, 261, generator=g)
    k = torch.arange(13, dtype=torch.float64) - 6 - 0.375
    f = torch.sinc(k) * torch.sinc(k / 7)
    return x, (f / f.sum()).float()


def real_fir_tolerance(x, f2, ref, pad, dtype):
    """u (fh fw + 2) sum |tap x| per element (+ 2^-8 |ref| in bf16), for an up = down = 1 launch."""
    from oracle import upfirdn as ou
    mag = ou.upfirdn2d(x.double().abs(), f2.abs(), padding=list(pad))
    tol = U * (f2.numel() + 2) * mag
    return tol + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0)
