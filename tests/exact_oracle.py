"""Exact-arithmetic oracle for the convolution / linear GEMM family (importable on the CPU).

With activations and weights in {-1, 0, +1} and bias, time embedding and residual small integers, every product of a
convolution is exact in bf16 x bf16 -> fp32, every partial sum is an integer below 2^24 - so fp32 accumulation is exact in ANY
order, across split-K slabs and a folded shortcut too - and a result of magnitude <= 256 is stored in bf16 unchanged.  A kernel
must then equal a float64 evaluation bit for bit, whatever its tiling, slicing or summation order: no tolerance.

conv_case() builds the operands of one ops.conv2d-style problem with its float64 reference and asserts the two conditions on the
reference itself: (a) max|y| <= 256, (b) for every sample and channel sum(y^2) < 2^24 (the GroupNorm partial sums are then exact
integers as well).  They are conditions, not measurements: a case that breaks one gets another seed or a lower density.
The launches that normalise such an output themselves (dense2.hip, afldm_af_act_slabs, the y_norm epilogue) are held to a
per-element tolerance on the same kind of operands by tests/fusednorm_oracle.py, which builds its chain cases with conv_case.
"""
import types

import torch
import torch.nn.functional as F

MAX_ABS = 256              # integers up to 2^8 are bf16 values
MAX_SUMSQ = 1 << 24        # integers below 2^24 are fp32 values
X_DENSITY = 0.5
K_FULL_DENSITY = 2304      # weight density min(0.5, 2304 / K): sigma(y)^2 = 0.5 * density * K <= 1152, sigma(y) <= 34


def ternary(shape, density, gen):
    """Values in {-1, 0, +1} (fp32), non-zero with probability `density`."""
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    keep = (torch.rand(shape, generator=gen) < density).float()
    return sign * keep


def small_ints(shape, lo, hi, gen):
    """Integers in [lo, hi] (fp32): bias, time embedding, residual."""
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def weight_density(K):
    return min(0.5, K_FULL_DENSITY / K)


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def reference(c, plain=False):
    """float64 NHWC result of the case `c` (the fields conv_case fills): F.conv2d in float64 of the concat x1 | x2, plus the 1x1
    shortcut, the broadcast time embedding and the residual.  plain: without bias, time embedding and residual (what split-K
    slabs sum to)."""
    if plain:
        c = types.SimpleNamespace(**{**vars(c), "bias": None, "temb": None, "residual": None})
    x = c.x1 if c.x2 is None else torch.cat([c.x1, c.x2], -1)
    x = _nchw(x)
    if c.form == "s2":
        lo, hi = c.pad
        x = F.pad(x, (lo, hi, lo, hi))
        stride, padding = 2, 0
    elif c.form == "up2":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        stride, padding = 1, 1
    else:
        stride, padding = 1, c.KS // 2
    bias = None if c.bias is None else c.bias.double()
    if c.per_sample_w:
        y = torch.cat([F.conv2d(x[b:b + 1], c.w[b].double().permute(0, 3, 1, 2), bias, stride=stride, padding=padding)
                       for b in range(x.shape[0])], 0)
    else:
        y = F.conv2d(x, c.w.double().permute(0, 3, 1, 2), bias, stride=stride, padding=padding)
    if c.shortcut is not None:
        sx1, sx2, sw = c.shortcut
        sx = sx1 if sx2 is None else torch.cat([sx1, sx2], -1)
        y = y + F.conv2d(_nchw(sx), sw.double().permute(0, 3, 1, 2))
    if c.temb is not None:
        cols = torch.arange(c.Cout) % c.temb.shape[1]
        y = y + c.temb.double()[:, cols][:, :, None, None]
    y = y.permute(0, 2, 3, 1).contiguous()
    if c.residual is not None:
        y = y + c.residual.double()
    return y


def check_caps(y64, what=""):
    """The two conditions on a float64 NHWC reference (see the module docstring)."""
    top = float(y64.abs().max())
    assert top <= MAX_ABS, f"{what}: max|y| = {top:.0f} > {MAX_ABS}: a bad case (another seed or a lower density), not a wider bound"
    sumsq = float((y64 * y64).flatten(1, -2).sum(1).max())
    assert sumsq < MAX_SUMSQ, f"{what}: sum(y^2) = {sumsq:.4g} >= 2^24 for some (sample, channel): a bad case"
    assert torch.equal(y64, y64.round()), f"{what}: the reference is not integral"
    return top, sumsq


def conv_case(B, H, W, C1, C2, Cout, KS=3, temb=False, temb_mod=0, residual=False, shortcut=None, per_sample_w=False,
              bias=True, form="same", pad=(1, 1), seed=0, w_density=None):
    """Operands (CPU fp32 NHWC / OHWI tensors holding small integers) and float64 reference of one problem:
      x1 | x2 [B, H, W, C1 | C2], w [Cout, KS, KS, C1 + C2] (per_sample_w: [B, Cout, KS, KS, C1 + C2]), bias [Cout],
      temb [B, temb_mod or Cout] (channel n takes column n % temb_mod), residual [B, Ho, Wo, Cout],
      shortcut = (sC1, sC2): a 1x1 convolution of sx1 | sx2 [B, H, W, sC1 | sC2] with sw [Cout, 1, 1, sC1 + sC2];
      form "same" (stride 1, KS 1 or 3), "s2" (stride 2 of x zero-padded by pad = (lo, hi)), "up2" (nearest x2, then 3x3 'same').
    Weight density min(0.5, 2304 / K), K = every reduced element (KS^2 (C1 + C2) + the shortcut's channels; the nearest-x2 form
    counts its folded taps, sums of up to four weights: 16 (C1 + C2))."""
    assert KS in (1, 3) and form in ("same", "s2", "up2")
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * (C1 + C2) + 31 * Cout + 7 * H + W + 131 * B)
    c = types.SimpleNamespace(B=B, H=H, W=W, C1=C1, C2=C2, Cout=Cout, KS=KS, form=form, pad=tuple(pad), temb_mod=temb_mod,
                              per_sample_w=per_sample_w)
    Csc = 0 if shortcut is None else shortcut[0] + shortcut[1]
    K = (16 if form == "up2" else KS * KS) * (C1 + C2) + Csc
    dens = weight_density(K) if w_density is None else w_density
    c.K, c.w_density = K, dens
    c.x1 = ternary((B, H, W, C1), X_DENSITY, gen)
    c.x2 = ternary((B, H, W, C2), X_DENSITY, gen) if C2 else None
    c.w = ternary(((B,) if per_sample_w else ()) + (Cout, KS, KS, C1 + C2), dens, gen)
    c.bias = small_ints((Cout,), -8, 8, gen) if bias else None
    c.temb = small_ints((B, temb_mod or Cout), -8, 8, gen) if temb else None
    Ho, Wo = (H // 2, W // 2) if form == "s2" else (2 * H, 2 * W) if form == "up2" else (H, W)
    c.residual = small_ints((B, Ho, Wo, Cout), -8, 8, gen) if residual else None
    c.shortcut = None
    if shortcut is not None:
        sC1, sC2 = shortcut
        c.shortcut = (ternary((B, H, W, sC1), X_DENSITY, gen), ternary((B, H, W, sC2), X_DENSITY, gen) if sC2 else None,
                      ternary((Cout, 1, 1, sC1 + sC2), dens, gen))
    c.ref = reference(c)
    c.what = (f"{form} B{B} {H}x{W} {C1}|{C2}->{Cout} KS{KS}" + (" temb" if temb else "") + (f"%{temb_mod}" if temb_mod else "")
              + (" res" if residual else "") + (f" sc{shortcut[0]}|{shortcut[1]}" if shortcut else "") + (" wB" if per_sample_w else ""))
    c.max_abs, c.max_sumsq = check_caps(c.ref, c.what)
    return c


def operands_survive(c, dtype):
    """True when every operand of the case is unchanged by a round trip through `dtype` (they are small integers)."""
    ts = [c.x1, c.x2, c.w, c.bias, c.temb, c.residual] + list(c.shortcut or ())
    return all(t is None or torch.equal(t.to(dtype).float(), t) for t in ts) and torch.equal(c.ref.to(dtype).double(), c.ref)


def assert_exact(got, ref64, what=""):
    """torch.equal(got.double().cpu(), ref64); on failure the count and the first mismatching (b, y, x, c) indices with both
    values - they show whether the fault is a seam, a halo, a tail or a sample index."""
    g = got.detach().double().cpu()
    assert g.shape == ref64.shape, f"{what}: shape {tuple(g.shape)} != {tuple(ref64.shape)}"
    if torch.equal(g, ref64):
        return
    bad = (g != ref64) | torch.isnan(g)
    idx = bad.nonzero()
    first = "; ".join(f"{tuple(int(v) for v in i)}: got {float(g[tuple(i)]):g} want {float(ref64[tuple(i)]):g}" for i in idx[:8])
    spans = ", ".join(f"dim{d} in [{int(idx[:, d].min())}, {int(idx[:, d].max())}]" for d in range(idx.shape[1]))
    raise AssertionError(f"{what}: {idx.shape[0]} of {g.numel()} values differ from the float64 reference ({spans}); first: {first}")


def assert_stats_exact(gn_partial, y, what=""):
    """gn_partial [B, S, C, 2] (per-channel partial sums and sums of squares of the stored output y [B, ..., C]): summed over the
    splits in float64 they must EQUAL sum(y) and sum(y^2) - every partial is an exact integer under the caps."""
    st = gn_partial.detach().double().cpu().sum(1)
    yd = y.detach().double().cpu()
    yd = yd.reshape(yd.shape[0], -1, yd.shape[-1])
    assert st.shape == (yd.shape[0], yd.shape[-1], 2), f"{what}: statistics shape {tuple(gn_partial.shape)}"
    assert_exact(st[..., 0], yd.sum(1), f"{what}: sum(y) from the statistics")
    assert_exact(st[..., 1], (yd * yd).sum(1), f"{what}: sum(y^2) from the statistics")


# ----------------------------------------------------------------------------------------------- case tables (kwargs of conv_case)
def _c(B, H, W, C1, C2, Cout, KS=3, **kw):
    return dict(B=B, H=H, W=W, C1=C1, C2=C2, Cout=Cout, KS=KS, **kw)


# the ragged shape of test_conv2d_every_gemm_variant: M = 288 is no tile multiple, virtual concat, Cout = 200
EVERY_VARIANT = _c(2, 12, 12, 128, 64, 200, residual=True)

# H3_CASES of tests/test_gpu_ops.py (conv3h.hip variants), batches cut to what fills two tiles
H3_EXACT = [
    # conv_case kwargs, variants
    (_c(1, 32, 32, 192, 0, 192, temb=True), (41, 46)),
    (_c(1, 32, 32, 384, 0, 192, residual=True), (41, 46)),
    (_c(1, 32, 32, 64, 0, 384, temb=True, residual=True), (41, 46)),
    (_c(2, 16, 16, 384, 0, 384, temb=True, residual=True), (43,)),
    (_c(2, 16, 16, 128, 0, 192), (43,)),
    (_c(3, 8, 8, 384, 0, 384, temb=True, residual=True), (51,)),
    (_c(3, 8, 8, 768, 0, 96, residual=True), (51,)),
    (_c(8, 4, 4, 768, 0, 768, temb=True, residual=True), (52,)),
    (_c(4, 4, 4, 256, 0, 96), (52,)),
    (_c(2, 16, 16, 384, 0, 96, temb=True, residual=True), (54,)),
    (_c(1, 32, 32, 192, 0, 288, temb=True, residual=True), (55,)),
]

# variant 58: 8 x 32 pixel blocks of planes larger than a tile (one non-square)
V58_EXACT = [
    _c(1, 64, 64, 128, 0, 128, temb=True, residual=True),
    _c(1, 72, 96, 64, 0, 256, residual=True),
    _c(1, 128, 128, 128, 0, 128),
]

# split-K: the 4^2, 8^2 and M = 48 shapes of test_conv2d_split_k_reduced_inside_the_launch with B <= 8
SPLITK_EXACT = [
    _c(8, 4, 4, 768, 0, 768, temb=True, residual=True),
    _c(8, 8, 8, 384, 0, 384, temb=True),
    _c(8, 8, 8, 768, 0, 384, residual=True),
    _c(3, 4, 4, 768, 0, 768, temb=True, residual=True),
]

# the folded 1x1 shortcut.  (plane, shortcut C1 | C2, Cout): SITES of test_gpu_shortcut_fold3.py (three filter taps per K step) ...
FOLD3_SITES = [(8, 768, 384, 384), (8, 384, 384, 384), (4, 768, 768, 768), (4, 768, 384, 768), (4, 384, 0, 768)]
# ... and the 16^2 / 32^2 sites of test_gpu_shortcut_fold.py (one tap per step at batch 64)
FOLD1_SITES = [(32, 384, 192, 192), (32, 192, 192, 192), (16, 384, 384, 384), (16, 384, 192, 384), (16, 192, 0, 384)]


def _fold_cases():
    """(N, C1, C2, Cout, B, dtype name, kind, forced variant): every case makes a folded call, and `kind` is the value
    afldm_conv2d_shortcut_ok must give for it - 1: one tap per K step, whole K per workgroup; 2: three taps per step.
      * batch 64, both dtypes: what the benchmark and the samplers run (kind 2 at 8^2 / 4^2, kind 1 at 16^2 / 32^2);
      * the small batches of the fold3 file (8^2: 2, 3; 4^2: 8, 4) and B = 3, 1 at 16^2 / 32^2 in bf16: the 96-cout small-batch
        tiles, all three-tap.  In fp32 no halo-patch tile takes a small batch (the planner keeps them on the GEMM tiles), so
        there is no fold to test and no case;
      * the one-tap tiles forced at small batches in both dtypes: variants 41 and 46 at 32^2 (B = 1), 43 at 16^2 (B = 2)."""
    out = []
    for s in FOLD3_SITES:
        out += [s + (64, dt, 2, None) for dt in ("fp32", "bf16")]
        out += [s + (b, "bf16", 2, None) for b in ((2, 3) if s[0] == 8 else (8, 4))]
    for s in FOLD1_SITES:
        out += [s + (64, dt, 1, None) for dt in ("fp32", "bf16")]
        out += [s + (b, "bf16", 2, None) for b in (3, 1)]
        for dt in ("fp32", "bf16"):
            out += [s + (1, dt, 1, v) for v in (41, 46)] if s[0] == 32 else [s + (2, dt, 1, 43)]
    return out


FOLD_CASES = _fold_cases()
# the split-K share cases of test_conv2d_shortcut_fold3_splitk_shares (4^2 planes, batch 64, 384 couts): dtype name, C1, C2, what
FOLD_SHARES = [("bf16", 128, 64, "boundary"), ("bf16", 128, 128, "uneven"), ("bf16", 128, 128, "boundary"),
               ("fp32", 96, 64, "uneven"), ("fp32", 64, 64, "boundary")]


def fold_case(N, C1, C2, Cout, B, seed=0):
    """conv3x3(h [B, N, N, Cout]) + conv1x1(x1 | x2): x1/x2 of the case are unused by the 3x3 (C1 = Cout, C2 = 0)."""
    return conv_case(B, N, N, Cout, 0, Cout, 3, shortcut=(C1, C2), seed=seed)


# operand plumbing: x1 | x2 seams at every C1 the FFHQ UNet concatenates at (its skip widths) and at the smallest the kernel takes
# (one K step: 64 bf16 / 32 fp32 channels)
SEAM_EXACT = [
    _c(2, 16, 16, 32, 32, 64), _c(2, 16, 16, 64, 64, 64),
    _c(2, 32, 32, 192, 192, 192, temb=True), _c(2, 16, 16, 384, 192, 384, temb=True), _c(2, 16, 16, 384, 384, 384),
    _c(2, 8, 8, 384, 384, 384, residual=True), _c(2, 8, 8, 768, 384, 384), _c(3, 4, 4, 768, 768, 768, temb=True),
    _c(3, 4, 4, 768, 384, 768), _c(3, 8, 8, 128, 128, 128, KS=1),
]

# tail shapes: the smallest at which each family can go wrong
TAIL_EXACT = {
    "cout96_3x5x7": _c(3, 5, 7, 64, 0, 96, temb=True),
    "conv_in_direct": _c(2, 12, 12, 4, 0, 64),
    "conv_in_mfma": _c(2, 32, 32, 4, 0, 192),
    "conv_out": _c(2, 32, 32, 192, 0, 4),
    "ragged_n_tile": _c(2, 16, 16, 128, 0, 200, residual=True),
    "ragged_n_tile_1x1": _c(3, 8, 8, 384, 0, 416, KS=1, temb=True),
}

# the resamplers: (form, pad, B, H, W, Cin, Cout) with even and odd plane sides (afldm_conv2d_s2 takes even input sides only: its
# odd sides are those of the OUTPUT, 5 x 7 and 3 x 5; afldm_conv2d_up2 takes couts in multiples of 64)
RESAMPLE_EXACT = [
    ("s2", (1, 1), 2, 16, 16, 128, 128), ("s2", (0, 1), 2, 16, 16, 128, 128), ("s2", (1, 1), 3, 10, 14, 64, 96),
    ("s2", (0, 1), 1, 32, 32, 128, 256), ("s2", (1, 1), 2, 6, 10, 64, 64), ("s2", (0, 1), 2, 6, 10, 64, 64),
    ("up2", None, 2, 8, 8, 128, 128), ("up2", None, 3, 5, 7, 64, 128), ("up2", None, 1, 16, 16, 256, 128),
    ("up2", None, 2, 3, 3, 64, 64),
]


def resample_case(form, pad, B, H, W, Cin, Cout, seed=0):
    return conv_case(B, H, W, Cin, 0, Cout, 3, form=form, pad=pad or (1, 1), seed=seed)


# the FFHQ UNet's widest reductions (the densities of the issue's table), checked on the CPU at B = 3
MODEL_SHAPES = [_c(3, 4, 4, 768, 768, 768), _c(3, 32, 32, 192, 0, 192), _c(3, 16, 16, 384, 0, 384), _c(3, 2, 2, 768, 0, 768),
                _c(3, 8, 8, 768, 0, 384)]


def static_cases():
    """(name, thunk) for every case the static tables above describe: the host test builds each (conv_case asserts the caps)."""
    out = [("every_variant", lambda: conv_case(**EVERY_VARIANT))]
    for i, (kw, _) in enumerate(H3_EXACT):
        out.append((f"h3[{i}]", lambda kw=kw: conv_case(**kw)))
    for name, table in (("v58", V58_EXACT), ("splitk", SPLITK_EXACT), ("seam", SEAM_EXACT), ("model", MODEL_SHAPES)):
        for i, kw in enumerate(table):
            out.append((f"{name}[{i}]", lambda kw=kw: conv_case(**kw)))
    for N, C1, C2, Cout, B in sorted({f[:5] for f in FOLD_CASES}):
        out.append((f"fold[{N}-{C1}|{C2}-{Cout}-B{B}]", lambda a=(N, C1, C2, Cout, B): fold_case(*a)))
    for dt, C1, C2, what in FOLD_SHARES:
        out.append((f"fold_shares[{dt}-{C1}|{C2}-{what}]", lambda a=(4, C1, C2, 384, 64): fold_case(*a)))
    for name, kw in TAIL_EXACT.items():
        out.append((f"tail[{name}]", lambda kw=kw: conv_case(**kw)))
    for r in RESAMPLE_EXACT:
        out.append((f"resample[{'-'.join(str(v) for v in r)}]", lambda r=r: resample_case(*r)))
    return out
