"""Integer-plane oracle for the fused convolution -> GroupNorm -> activation launches (importable on the CPU).

Three launches normalise a convolution's own output inside the launch that finishes it: afldm_conv2x2_const_norm_act (dense2.hip),
afldm_af_act_slabs (k_af_act_slabs, af.hip) and the y_norm epilogue of the one-sample 8x8 halo tile (conv3h_body.inc).  The argument
of tests/exact_oracle.py carries over: feed the producer small integers and the value it stores and normalises is exact; the group
sums are then exact integers as well (sum(y^2) < 2^24), so (mean, variance) do not depend on the order of summation.  What is left
is fp32 arithmetic on O(1) numbers and one rounding to the storage type - a tolerance per ELEMENT, about one half-ulp wide:

    bf16   |got - ref| <= 2^-8 |ref| + A,   A = 2^-16 max|hn|     (hn: the case's normalised tensor)
    fp32   |got - ref| <= 2e-5 max|ref|                            (the project's fp32 class)

2^-8 |ref| is the half-ulp of the one bf16 store.  A covers the fp32 arithmetic in front of it: the float32 restatements below
(model_slabs, model_dense2, model_ynorm) stay within 2^-21 max|hn| of float64 (asserted at A / 8 by the host file); the factor of 32
is for the device's silu_f (hardware exp2 and reciprocal, one unit in the last place each) and for fused-multiply-add contraction.
Raw outputs (want_raw, y) are exact quantities: torch.equal.

References are plain float64 from the integer operands: group_norm64 over cpg channels x N^2 pixels, warped64 = D silu(U x U^T) D^T
with the VALUES of the fp32 matrices the kernels are handed (filters(N): afldm_filter_matrix, what ops.filter_matrices uploads) taken
to float64, so the filters' own rounding is not charged to the kernel; the host file holds those matrices to
oracle.ideal_filters.up_matrix / down_matrix.

Conditions, asserted on the reference before anything runs (check_conditions) - conditions, not measurements; a case that breaks
one gets another seed or density, never a wider bound: exact_oracle.check_caps (|y| <= 256, sum(y^2) < 2^24, integral), every
group's variance >= 1 and every group's sigma <= 12 (a unit fault in y is then at least 1/12 of a normalised unit).
"""
import functools
import types

import torch

import exact_oracle as xo

EPS = 1e-5
BF16, FP32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": FP32}
MIN_VAR, MAX_SIGMA = 1.0, 12.0
D2_ROWS, D2_WAVES = 16, 8                 # dense2.hip: samples per workgroup, K slices (waves)


def kpf(dtype):
    """k elements of one MFMA K step (common.hpp Mma<T>::KPF)."""
    return 32 if dtype == BF16 else 16


# ------------------------------------------------------------------------------------------------------------------ references
@functools.lru_cache(None)
def filters(N):
    """(U [2N, N], D [N, 2N]) fp32: the matrices ops.filter_matrices(N) hands the kernels (host copies)."""
    from afldm_amd import _lib
    return _lib.filter_matrix(0, N, 2), _lib.filter_matrix(1, 2 * N)


def group_norm64(y, gamma, beta, G, eps=EPS):
    """y [B, P, C] -> (hn [B, P, C], mean [B, G], var [B, G]) in float64 over cpg channels x P pixels (biased variance)."""
    B, P, C = y.shape
    v = y.double().reshape(B, P, G, C // G)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    hn = ((v - mean) / (var + eps).sqrt()).reshape(B, P, C) * gamma.double() + beta.double()
    return hn, mean.reshape(B, G), var.reshape(B, G)


def warped64(hn, N):
    """WarpedNonlinearity(SiLU) of hn [B, N * N, C] (pixel = N h + w): D silu(U x U^T) D^T in float64."""
    U, D = (m.double() for m in filters(N))
    B, P, C = hn.shape
    up = torch.einsum("ph,bhwc,qw->bpqc", U, hn.reshape(B, N, N, C), U)
    s = up * torch.sigmoid(up)
    return torch.einsum("hp,bpqc,wq->bhwc", D, s, D).reshape(B, P, C)


def plane_constant(out, what=""):
    """out [B, 4, C] of an N = 2 activation: the four pixels of a plane agree to 1e-12 (lpf(4) = [1, 0, 0, 0]); one of them."""
    spread = float((out - out[:, :1]).abs().max())
    assert spread <= 1e-12, f"{what}: the reference's 2x2 plane is not constant ({spread:.3g})"
    return out[:, 0]


def check_conditions(y, G, what=""):
    """y [B, P, C] float64: the caps of exact_oracle and the variance window of every (sample, group).  -> (min var, max sigma)"""
    xo.check_caps(y, what)
    _, _, var = group_norm64(y, torch.ones(y.shape[-1]), torch.zeros(y.shape[-1]), G)
    lo, hi = float(var.min()), float(var.max()) ** 0.5
    assert lo >= MIN_VAR, f"{what}: a group's variance is {lo:.3g} < 1: a bad case (another seed or density), not a wider bound"
    assert hi <= MAX_SIGMA, f"{what}: a group's sigma is {hi:.3g} > 12: a bad case (another seed or density), not a wider bound"
    return lo, hi


def tolerance(ref, hn, dtype):
    ref = ref.double()
    if dtype == BF16:
        return ref.abs() * 2.0 ** -8 + 2.0 ** -16 * float(hn.abs().max())
    return torch.full_like(ref, 2e-5 * float(ref.abs().max()))


def check_elements(got, ref, hn, dtype, what=""):
    """Every element of `got` within the tolerance of the float64 `ref` (module docstring).  On failure: the count, the worst
    (b, pixel, c) with both values, and error / tolerance.  Returns the worst error / tolerance."""
    g = got.detach().double().cpu()
    assert g.numel() == ref.numel(), f"{what}: shape {tuple(g.shape)} against {tuple(ref.shape)}"
    g = g.reshape(ref.shape)
    ratio = torch.nan_to_num((g - ref.double()).abs() / tolerance(ref, hn, dtype), nan=float("inf"))
    worst = float(ratio.max())
    if worst > 1.0:
        bad = int((ratio > 1.0).sum())
        i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f"{what} {dtype}: {bad} of {g.numel()} elements outside the tolerance; worst at (b, pixel, c) = {i}: got "
                             f"{float(g[i]):.9g} want {float(ref[i]):.9g}, error / tolerance = {worst:.3g}")
    return worst


def rel_rms(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------- float32 restatement: shared pieces
def _store(x, dtype):
    """One rounding to the storage type, read back as fp32."""
    return x.to(dtype).float()


def _finish32(r, gamma, beta, G, eps, stats_of=None, group_shift=0, chan_shift=0):
    """r [B, P, C] fp32 (the stored convolution output) -> X fp32: per-channel fp32 sums, an fp64 finish per group
    (gn_mean_rstd, common.hpp), scale / shift in fp32.  stats_of: the tensor the sums are taken over (a planted fault);
    group_shift / chan_shift: another group's (mean, rstd) / another channel's gamma, beta (planted faults)."""
    B, P, C = r.shape
    cpg = C // G
    s = r if stats_of is None else stats_of
    n = s.shape[1] * (s.shape[2] // G)
    s1 = s.sum(1).double().reshape(B, G, -1).sum(2)
    s2 = (s * s).sum(1).double().reshape(B, G, -1).sum(2)
    m = s1 / n
    var = (s2 / n - m * m).float().clamp_min(0)
    mean, rstd = m.float(), 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=FP32))
    mean, rstd = mean.roll(-group_shift, 1), rstd.roll(-group_shift, 1)
    gm, bt = gamma.float().roll(-chan_shift), beta.float().roll(-chan_shift)
    sc = rstd.repeat_interleave(cpg, 1) * gm
    sh = bt - mean.repeat_interleave(cpg, 1) * sc
    return r * sc[:, None] + sh[:, None]


def _warped32(X, N):
    U, D = filters(N)
    B, P, C = X.shape
    up = torch.einsum("ph,bhwc,qw->bpqc", U, X.reshape(B, N, N, C), U)
    s = up * (1.0 / (1.0 + torch.exp(-up)))
    return torch.einsum("hp,bpqc,wq->bhwc", D, s, D).reshape(B, P, C)


def _swap12(t):
    """Pixels 1 and 2 of every plane exchanged ([B, P, C])."""
    t = t.clone()
    t[:, [1, 2]] = t[:, [2, 1]]
    return t


# ---------------------------------------------------------------------------------------------- recipe 1: dictated slabs
# (nslab, N, act, C, G, temb, residual, want_raw, bias).  temb: None, "zero" (temb_stride 0: one row for all samples), "cout"
# (a row of C per sample), "wide" (a slice of a wider row: temb_stride > C, as the step table gives); act 2: the plane-constant
# [B, C] form (N = 2).  (C, G) -> threads per workgroup: (768, 32) 192, (192, 32) 192, (96, 8) 96, (64, 8) 64, (256, 1) 256, (48, 16) 48
SLAB_B = 3
SLAB_CG = [(768, 32), (192, 32), (96, 8), (64, 8), (256, 1), (48, 16)]
SLAB_NSLAB = [1, 3, 4, 5, 9]
TEMB_MODES = [None, "zero", "cout", "wide"]


def _slab_table():
    rows, i = [], 0
    for C, G in SLAB_CG:
        for N, act in ((2, 0), (2, 1), (2, 2), (4, 0), (4, 1)):
            rows.append((SLAB_NSLAB[(i + i // 5) % 5], N, act, C, G, TEMB_MODES[(i + i // 4) % 4], (i // 3) % 2 == 0, (i // 2) % 2 == 1, i % 7 != 3))
            i += 1
    return rows


# ... and the model's own class at batch 64 (4^2 planes, 24 channels per group, two slices: tests/test_fusednorm_oracle_host.py)
SLAB_CASES = _slab_table() + [(2, 4, 1, 768, 32, "cout", False, False, True), (2, 4, 0, 768, 32, None, True, True, True)]


def _temb(mode, B, C, lo, hi, gen):
    """(integer temb as the kernel sees it, temb_stride, its [B, C] float64 meaning, the tensor to upload, the first column of the
    kernel's view in it)."""
    if mode is None:
        return None, 0, torch.zeros(B, C, dtype=torch.float64), None, 0
    if mode == "zero":
        t = xo.small_ints((C,), lo, hi, gen)
        return t, 0, t.double().expand(B, C), t, 0
    if mode == "cout":
        t = xo.small_ints((B, C), lo, hi, gen)
        return t, C, t.double(), t, 0
    wide = xo.small_ints((B, 2 * C + 24), lo, hi, gen)          # the step table's row: this block's slice starts at column C + 8
    t = wide[:, C + 8:2 * C + 8]
    return t, wide.shape[1], t.double(), wide, C + 8


@functools.lru_cache(None)
def slab_case(nslab, N, act, C, G, temb, residual, want_raw, bias, B=SLAB_B, seed=0):
    """y[b, px, c] = m[b, g] + s[b, g] t[b, px, c]: integer m in [-16, 16], s in {1, 2, 4, 8}, t in [-3, 3] drawn per group until
    its variance lies in [1, 2.25] (variance of y in [1, 144] whatever s is) - every (sample, group) has its own mean and
    deviation.  Bias, temb and residual are integers in [-8, 8] and are INCLUDED in y: the slabs sum to y - bias - temb -
    residual, split into `nslab` integer slabs with signs mixed.  gamma in [0.5, 1.5], beta ~ 0.3 N(0, 1), fp32, per channel."""
    gen = torch.Generator().manual_seed(7 + 1000003 * seed + 31 * C + 7 * G + 3 * N + nslab + 101 * act)
    P, cpg = N * N, C // G
    c = types.SimpleNamespace(nslab=nslab, N=N, act=act, C=C, G=G, B=B, P=P, temb_mode=temb, want_raw=want_raw, eps=EPS)
    m = torch.randint(-16, 17, (B, 1, G, 1), generator=gen).double()
    s = (2 ** torch.randint(0, 4, (B, 1, G, 1), generator=gen)).double()
    pmf = torch.tensor([0.10, 0.15, 0.25, 0.0, 0.25, 0.15, 0.10])
    t = torch.zeros(B, P, G, cpg, dtype=torch.float64)
    todo = torch.ones(B, G, dtype=torch.bool)
    for _ in range(200):
        if not todo.any():
            break
        draw = (torch.multinomial(pmf, B * P * G * cpg, True, generator=gen) - 3).double().reshape(B, P, G, cpg)
        draw = torch.where(torch.rand(B, P, G, cpg, generator=gen) < 0.4, torch.zeros(()).double(), draw)
        v = draw.var((1, 3), unbiased=False)
        ok = todo & (v >= 1.0) & (v <= 2.25)
        t = torch.where(ok[:, None, :, None], draw, t)
        todo &= ~ok
    assert not todo.any(), "no admissible t for some group"
    c.y = (m + s * t).reshape(B, P, C)
    c.bias = xo.small_ints((C,), -8, 8, gen) if bias else None
    c.temb, c.temb_stride, temb64, c.temb_full, c.temb_col0 = _temb(temb, B, C, -8, 8, gen)
    c.residual = xo.small_ints((B, P, C), -8, 8, gen) if residual else None
    rest = c.y - temb64[:, None] - (0 if c.bias is None else c.bias.double()) - (0 if c.residual is None else c.residual.double())
    parts = [torch.randint(-64, 65, (B, P, C), generator=gen).double() for _ in range(nslab - 1)]
    parts.append(rest - sum(parts))
    c.slabs = torch.stack(parts).float().reshape(nslab, B * P, C)
    assert torch.equal(c.slabs.double().sum(0).reshape(B, P, C), rest)
    c.gamma = (torch.rand(C, generator=gen) + 0.5).float()
    c.beta = (torch.randn(C, generator=gen) * 0.3).float()
    c.what = f"slabs z{nslab} N{N} act{act} C{C}/G{G} temb={temb} res={int(residual)} raw={int(want_raw)} bias={int(bias)}"
    c.min_var, c.max_sigma = check_conditions(c.y, G, c.what)
    c.hn, _, _ = group_norm64(c.y, c.gamma, c.beta, G)
    c.ref = finish64(c.hn, N, act, c.what)
    return c


def finish64(hn, N, act, what=""):
    """The launch's output in float64 from the normalised tensor: act 0 hn itself, 1 the activation, 2 its plane-constant form."""
    if act == 0:
        return hn
    out = warped64(hn, N)
    return plane_constant(out, what) if act == 2 else out


def model_slabs(c, dtype, fault=None, slabs=None, bias=None, temb64=None):
    """k_af_act_slabs in float32: slabs added in order, + bias + temb + residual, ONE rounding to `dtype` (raw), per-plane sums in
    fp32, the group's in fp64, scale / shift, activation.  -> (out before the store [fp32], out as stored, raw as stored).
    Planted faults: "slab_skipped" (slab 4 is never added), "pixswap", "temb_row" (sample b + 1's row), "group_stats" (group g + 1's
    mean and rstd), "gamma_beta" (channel n + 1's), "residual_late" (the value is rounded and its sums are taken before the residual
    joins it: on integers the rounding itself is exact, so only the statistics show it)."""
    B, P, C = c.B, c.P, c.C
    v = torch.zeros(B * P, C)
    for z in range(c.nslab):
        if fault == "slab_skipped" and z == 4:
            continue
        v = v + c.slabs[z]
    v = v.reshape(B, P, C)
    if c.bias is not None:
        v = v + c.bias
    if c.temb is not None:
        t = c.temb.float().expand(B, C) if c.temb_stride == 0 else c.temb.float()
        v = v + (t.roll(-1, 0) if fault == "temb_row" else t)[:, None]
    stats_of = None
    if c.residual is not None:
        if fault == "residual_late":
            stats_of = _store(v, dtype)
        v = v + c.residual
    r = _store(v, dtype)
    if fault == "pixswap":
        r = _swap12(r)
    X = _finish32(r, c.gamma, c.beta, c.G, c.eps, stats_of, 1 if fault == "group_stats" else 0, 1 if fault == "gamma_beta" else 0)
    out = X if c.act == 0 else _warped32(X, c.N)
    if c.act == 2:
        out = out[:, 0]
    return out, _store(out, dtype), r


# ---------------------------------------------------------------------------------------------- recipe 2: dense2
# (B, K steps per wave or -Cin, Cout, G, temb, bias, weights).  K steps n: Cin = 256 n in bf16, 128 n in fp32 - 1, 2, 3 a ragged
# first register group (three steps per group), 4 and 6 the second trip of the double-buffered loop (6: both buffers full), 7 and 13
# the third (a lone step, ragged); negative: Cin itself (the model's sites 768 -> 768 and 1536 -> 768, G = 32: 3 and 6 steps in bf16,
# 6 and 12 in fp32).
# weights "conv": a ternary nn.Conv2d through blocks.packed_conv_dense2x2_const_cm (tap sums of four weights), "ints": dictated
# integers in [-4, 4].  B: 1 (one row tile: the non-temporal weight loads), 16, 17 and 33 (row tiles whose tail rows repeat the
# last sample).  Bias and temb integers in [-3, 3] (they widen the group's variance; the window is the condition).
DENSE2_CASES = [
    (1, 1, 64, 8, None, True, "conv"), (16, 1, 96, 8, "zero", True, "ints"), (17, 2, 192, 8, "cout", True, "conv"),
    (33, 2, 64, 8, "wide", True, "ints"), (1, 3, 96, 8, "cout", False, "ints"), (16, 3, 192, 8, "wide", True, "conv"),
    (17, 4, 64, 8, "zero", True, "ints"), (33, 4, 96, 8, None, True, "conv"), (1, 6, 192, 8, "wide", True, "ints"),
    (16, 6, 64, 8, "cout", True, "conv"), (17, 7, 96, 8, "wide", False, "conv"), (33, 7, 192, 8, "zero", True, "ints"),
    (1, 13, 64, 8, "zero", True, "conv"), (17, 13, 192, 8, None, True, "ints"), (33, 13, 96, 8, "cout", True, "ints"),
    (16, 13, 64, 8, "wide", False, "ints"), (33, -768, 768, 32, "cout", True, "conv"), (16, -768, 768, 32, "zero", True, "ints"),
    (1, 2, 192, 8, None, False, "conv"), (17, -768, 768, 32, "wide", True, "ints"), (16, -1536, 768, 32, "cout", True, "conv"),
]
D2_VARIANCE = 32.0           # of the GEMM part of y: 0.5 Cin E[w^2]


def dense2_cin(steps, dtype):
    return -steps if steps < 0 else steps * D2_WAVES * kpf(dtype)


def tap_sum_cm(W):
    """[Cout, Cin, 3, 3] -> [4 Cout, Cin] float64, row = 4 n + pixel: the tap sums a plane-constant 2x2 input sees
    (pixel (oh, ow): taps [1 - oh : 3 - oh, 1 - ow : 3 - ow]) - what blocks.packed_conv_dense2x2_const_cm must pack bit for bit."""
    W = W.double()
    blocks = [W[:, :, 1 - oh:3 - oh, 1 - ow:3 - ow].sum((2, 3)) for oh in (0, 1) for ow in (0, 1)]
    return torch.stack(blocks, 1).reshape(4 * W.shape[0], -1)


@functools.lru_cache(None)
def dense2_case(B, steps, Cout, G, temb, bias, weights, dtype, seed=0):
    Cin = dense2_cin(steps, dtype)
    gen = torch.Generator().manual_seed(11 + 1000003 * seed + 31 * Cin + 7 * Cout + 131 * B)
    c = types.SimpleNamespace(B=B, Cin=Cin, Cout=Cout, G=G, cpg=Cout // G, dtype=dtype, temb_mode=temb, weights=weights, eps=EPS,
                              N=2, P=4, C=Cout, act=2, conv_w=None)
    c.a = xo.ternary((B, Cin), 0.5, gen)
    if weights == "conv":
        c.conv_w = xo.ternary((Cout, Cin, 3, 3), D2_VARIANCE / (2.0 * Cin), gen)      # E[tap sum^2] = 4 density
        w = tap_sum_cm(c.conv_w)
    else:
        keep = torch.rand(4 * Cout, Cin, generator=gen) < D2_VARIANCE / (3.75 * Cin)   # E[w^2] = 7.5 density
        mag = torch.randint(1, 5, (4 * Cout, Cin), generator=gen) * (torch.randint(0, 2, (4 * Cout, Cin), generator=gen) * 2 - 1)
        w = (mag * keep).double()
    c.w_cm = w.float()
    c.bias = xo.small_ints((Cout,), -3, 3, gen) if bias else None
    c.temb, c.temb_stride, temb64, c.temb_full, c.temb_col0 = _temb(temb, B, Cout, -3, 3, gen)
    y = (c.a.double() @ w.t()).reshape(B, Cout, 4).permute(0, 2, 1)                   # [B, pixel, Cout]
    c.y = (y + temb64[:, None] + (0 if c.bias is None else c.bias.double())).contiguous()
    c.gamma = (torch.rand(Cout, generator=gen) + 0.5).float()
    c.beta = (torch.randn(Cout, generator=gen) * 0.3).float()
    c.what = f"dense2 B{B} {Cin}->{Cout}/G{G} temb={temb} bias={int(bias)} w={weights}"
    c.min_var, c.max_sigma = check_conditions(c.y, G, c.what)
    c.hn, _, _ = group_norm64(c.y, c.gamma, c.beta, G)
    c.ref = finish64(c.hn, 2, 2, c.what)
    for t in (c.a, c.w_cm, c.temb):
        assert t is None or torch.equal(t.to(dtype).float(), t)
    return c


def model_dense2(c, fault=None, where=None):
    """k_dense2_gn_act in float32: eight K slices in steps of KPF elements, added in wave order; + bias + temb; ONE rounding; per-tile
    fp32 sums (16 columns = 4 channels x 4 pixels), fp64 finish over the group's NT tiles; scale / shift; the N = 2 activation.
    -> (out before the store, out as stored).  Planted faults, at where = (group, tile, row tile): "kstep" (one K step of wave 5's
    slice dropped for the tile's 16 columns), "kelem" (one k element dropped for one column); in the workgroup (group, row tile):
    "tiles" (the group's sums over NT - 1 tiles), "temb_row", "group_stats", "gamma_beta" (as in model_slabs)."""
    B, Cin, Cout, cpg, dtype = c.B, c.Cin, c.Cout, c.cpg, c.dtype
    KW, step = Cin // D2_WAVES, kpf(c.dtype)
    a, w = c.a, c.w_cm
    acc = torch.zeros(B, 4 * Cout)
    for wave in range(D2_WAVES):
        part = torch.zeros(B, 4 * Cout)
        for ks in range(KW // step):
            k0 = wave * KW + ks * step
            part = part + a[:, k0:k0 + step] @ w[:, k0:k0 + step].t()
        acc = acc + part
    g, t, rt = where if where is not None else (0, 0, 0)
    rows = slice(rt * D2_ROWS, min(B, (rt + 1) * D2_ROWS))
    cols = slice(4 * (g * cpg + 4 * t), 4 * (g * cpg + 4 * t) + 16)
    if fault == "kstep":
        k0 = 5 * KW + (KW // step - 1) * step
        acc[rows, cols] -= a[rows, k0:k0 + step] @ w[cols, k0:k0 + step].t()
    if fault == "kelem":
        hit = (a[rows, :, None] * w[cols].t()[None]).abs().sum(0).nonzero()[0]       # (k, column) with a non-zero product
        k, col = int(hit[0]), cols.start + int(hit[1])
        acc[rows, col] -= a[rows, k] * w[col, k]
    v = acc.reshape(B, Cout, 4).permute(0, 2, 1)
    if c.bias is not None:
        v = v + c.bias

    def tail(f):
        u = v
        if c.temb is not None:
            tt = c.temb.float().expand(B, Cout) if c.temb_stride == 0 else c.temb.float()
            u = u + (tt.roll(-1, 0) if f == "temb_row" else tt)[:, None]
        r = _store(u, dtype)
        stats_of = r.reshape(B, 4, c.G, cpg)[..., :cpg - 4].reshape(B, 4, -1) if f == "tiles" else None
        X = _finish32(r, c.gamma, c.beta, c.G, c.eps, stats_of, 1 if f == "group_stats" else 0, 1 if f == "gamma_beta" else 0)
        return _warped32(X, 2)[:, 0]

    out = tail(None)
    if fault in ("temb_row", "tiles", "group_stats", "gamma_beta"):         # confined to the workgroup (group g, row tile rt)
        out[rows, g * cpg:(g + 1) * cpg] = tail(fault)[rows, g * cpg:(g + 1) * cpg]
    return out, _store(out, dtype)


# ---------------------------------------------------------------------------------------------- recipe 3: chain and y_norm
# exact_oracle.conv_case with its w_density chosen per case: the convolution part of y gets a variance of ~ 24 beside the integer
# bias, time embedding and residual (variance 24 each), sigma ~ 8.5.
def chain_density(K):
    return 48.0 / K


# (B, N, Cin, Cout, shortcut): conv2d_slabs -> af_act_slabs.  The last row is the 4^2 site of tests/test_gpu_shortcut_fold3.py whose
# slabs carry the folded 1x1 shortcut (no residual then)
CHAIN_CASES = [(8, 2, 768, 768, None), (8, 4, 768, 768, None), (64, 4, 1536, 768, None), (64, 4, 768, 768, (384, 0))]
CHAIN_G = 32


@functools.lru_cache(None)
def chain_case(B, N, Cin, Cout, shortcut, seed=0):
    """One convolution with bias, time embedding and (no shortcut) residual, finished two ways from the same slabs:
      "act":  + bias + temb             -> GroupNorm -> activation   (conv1 -> norm2 of a ResnetBlock2D), act = 1
      "norm": + bias + residual, raw    -> GroupNorm only            (conv2 -> Attention.group_norm),    act = 0
    (with a folded shortcut: + bias only, twice).  -> the conv_case with .plain (float64 slab sum) and .fin[kind] = (y, hn, ref)."""
    K = 9 * Cin + (0 if shortcut is None else sum(shortcut))
    c = xo.conv_case(B, N, N, Cin, 0, Cout, 3, temb=True, residual=shortcut is None, shortcut=shortcut, seed=seed,
                     w_density=chain_density(K))
    gen = torch.Generator().manual_seed(13 + Cin + B + N)
    c.gamma = (torch.rand(Cout, generator=gen) + 0.5).float()
    c.beta = (torch.randn(Cout, generator=gen) * 0.3).float()
    P = N * N
    full = c.ref.reshape(B, P, Cout)
    temb = c.temb.double()[:, None]
    res = 0 if c.residual is None else c.residual.double().reshape(B, P, Cout)
    c.plain = full - c.bias.double() - temb - res
    c.fin = {}
    for kind, y, act in (("act", full - res, 1), ("norm", full - temb, 0)):
        check_conditions(y, CHAIN_G, f"{c.what} {kind}")
        hn, _, _ = group_norm64(y, c.gamma, c.beta, CHAIN_G)
        c.fin[kind] = (y, hn, finish64(hn, N, act))
    return c


# y_norm (8^2 planes, bf16, variant 51 with the whole K per workgroup): (B, Cin, Cout, G, shortcut, temb).  afldm_conv2d_norm_ok accepts, among
# Cin = Cout in {96, 192, 384, 768} and G in {8, 32}: 192 from batch 54, 384 from batch 41 (with the folded 768-channel shortcut too),
# 768 from batch 21 but not at 64 (another tile takes it there), 96 never; G plays no part.  NORM_OK_FROM holds the first batch.
NORM_OK_FROM = {192: 54, 384: 41, 768: 21}
# temb: a time embedding beside the bias (with few channels per group the two integer offsets alone can pass sigma = 12)
YNORM_CASES = [(41, 384, 384, 32, None, False), (64, 384, 384, 8, None, True), (41, 384, 384, 32, (384, 384), False),
               (54, 192, 192, 8, None, True), (64, 192, 192, 32, None, False), (21, 768, 768, 32, None, True)]


@functools.lru_cache(None)
def ynorm_case(B, Cin, Cout, G, shortcut, temb, seed=0):
    K = 9 * Cin + (0 if shortcut is None else sum(shortcut))
    c = xo.conv_case(B, 8, 8, Cin, 0, Cout, 3, temb=temb, residual=False, shortcut=shortcut, seed=seed,
                     w_density=chain_density(K))
    add_norm(c, G)
    check_conditions(c.y3, G, c.what)
    return c


def add_norm(c, G, seed=17):
    """Per-channel gamma / beta and the float64 GroupNorm of the case's reference: c.hn [B, P, Cout] (conditions asserted apart)."""
    gen = torch.Generator().manual_seed(seed + c.Cout + G)
    c.G = G
    c.gamma = (torch.rand(c.Cout, generator=gen) + 0.5).float()
    c.beta = (torch.randn(c.Cout, generator=gen) * 0.3).float()
    c.y3 = c.ref.reshape(c.B, -1, c.Cout)
    c.hn, _, c.var = group_norm64(c.y3, c.gamma, c.beta, G)
    return c


def model_ynorm(c, dtype=BF16, fault=None):
    """The y_norm epilogue in float32 from the stored (exact) y: per-channel fp32 sums, fp64 finish per group, scale / shift, one
    rounding.  Planted faults: "pixswap", "group_stats", "gamma_beta"."""
    r = _store(c.y3.float(), dtype)
    if fault == "pixswap":
        r = _swap12(r)
    X = _finish32(r, c.gamma, c.beta, c.G, EPS, None, 1 if fault == "group_stats" else 0, 1 if fault == "gamma_beta" else 0)
    return X, _store(X, dtype)


def all_cases():
    """(name, thunk) of every case the GPU file lists (the host file builds each: the conditions are asserted in the builders)."""
    out = []
    for i, row in enumerate(SLAB_CASES):
        out.append((f"slabs[{i}]", lambda row=row: slab_case(*row)))
    for dt in ("fp32", "bf16"):
        for i, row in enumerate(DENSE2_CASES):
            out.append((f"dense2[{dt}-{i}]", lambda row=row, dt=dt: dense2_case(*row, DT[dt])))
    for i, row in enumerate(CHAIN_CASES):
        out.append((f"chain[{i}]", lambda row=row: chain_case(*row)))
    for i, row in enumerate(YNORM_CASES):
        out.append((f"ynorm[{i}]", lambda row=row: ynorm_case(*row)))
    return out
