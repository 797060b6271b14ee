"""GroupNorm partial sums on MI355X: every producer split and every consumer finish, against tests/gn_oracle.py.

Producers (afldm_gn_stats, afldm_gn_fold) are checked bit for bit on integer planes, whose sums are exact in any order.  Consumers
(afldm_gn_apply, afldm_af_act and its forms, afldm_gn_table, the fused launches) are handed hand-made partials - ragged cuts,
split counts from the matrix below, S1 != S2 on a concat - of data in which every (sample, group) has its own mean and standard
deviation, and are compared with the float64 finish of the SAME partials: what is left is the kernel's own arithmetic.

What each part would catch, reasoned from the code (csrc/common.hpp, csrc/gn.hip, csrc/af.hip); test_gn_oracle_host plants the
first four on the CPU, in this file's own cases, and shows that each leaves the bound asserted here:
  a stats load indexed with another sample    every consumer case: B = 3 and each (b, g) has its own mean (an O(ratio) change)
  `sp < S` masking with S1 != S2              the concat cases at (1, 32), (9, 4), (32, 3): gn_group_sums_wave / gn_wave_keys and
                                              the three copies in k_af_act_plane read past a tensor's last split (another sample's
                                              partials, or past the buffer for the last sample) - test_af_act_splits[*-concat*]
  the S % 8 tail of gn_channel_sums           S = 1, 3, 9, 17 (tail only, 8 + 1, 16 + 1) in test_gn_apply_splits and the
                                              gn_channel_sums users behind it (conv_out_fused)
  a k_gn_partial split boundary               test_gn_stats_exact at HW = 63, 65, 255, 257, 1023, 1025 (HW % S != 0), per split
  the second round g0 += 32                   test_gn_apply_splits[(96, 0, 48, 64)] and (64, 0, 64, 4)
  the fmaxf(var, 0) clamp                     the starved variants: a NaN at ratio 32 with the loud constant (gn_apply, gn_table),
                                              4e-4 in k against 4 u with the quiet one (gn_table)
"""
import pytest
import torch

import gn_oracle as go
from test_gpu_ops import close

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
BF16 = torch.bfloat16
B3 = 3
EPS = 1e-5
SINGLE_S = [1, 3, 8, 9, 17, 32]
CONCAT_S = [(1, 32), (9, 4), (8, 8), (32, 3)]
# (ratio, starved, constant): hard planes at ratio 8 and 32 and the starved variant
VARIANTS = [(8, False, 0.25), (32, False, 0.25), (32, True, 0.25)]
LOUD = [(8, False, "loud"), (32, False, "loud"), (32, True, "loud")]       # only with the element-wise bound


def _ops():
    from afldm_amd import ops
    return ops


def _id(v):
    return str(v).replace("torch.", "")


def _affine(C, seed):
    gen = torch.Generator().manual_seed(1000 + seed)
    return 1 + 0.2 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)


class Case:
    """Hard planes x [B, HW, C1 + C2] with hand-made partials of each half and the float64 finish of exactly those."""

    def __init__(self, B, C1, C2, G, HW, dtype, ratio, starve, const, S1, S2, seed=0, eps=EPS):
        C = C1 + C2
        self.B, self.C1, self.C2, self.C, self.G, self.HW, self.dtype, self.eps = B, C1, C2, C, G, HW, dtype, eps
        self.x = go.hard_planes(B, C, G, HW, ratio, 17 * seed + C + HW, dtype, const=const)
        self.gamma, self.beta = _affine(C, seed)
        self.set_splits(S1, S2, starve, seed)

    def set_splits(self, S1, S2, starve, seed=0):
        x, C1, C = self.x, self.C1, self.C
        self.st1 = go.partials(x[..., :C1].contiguous(), go.ragged_cuts(self.HW, S1, 100 * seed + S1))
        self.st2 = go.partials(x[..., C1:].contiguous(), go.ragged_cuts(self.HW, S2, 100 * seed + 50 + S2)) if self.C2 else None
        if starve:
            self.st1 = go.starved(self.st1, self.G, C, 0)
            self.st2 = go.starved(self.st2, self.G, C, C1) if self.C2 else None
        self.mean, self.rstd = go.finish(self.st1, self.st2, self.G, self.HW * C // self.G, self.eps)
        self.ref = go.apply(x, self.mean, self.rstd, self.gamma, self.beta, self.G)          # [B, HW, C] float64
        self.k, self.sh = go.scale_shift(self.mean, self.rstd, self.gamma, self.beta, self.G)
        return self

    def dev(self, shape=None):
        """(x1, x2, GNStats, gamma, beta) on the GPU; x as [B, *shape, C] (default [B, HW, 1, C])."""
        ops = _ops()
        shape = (self.HW, 1) if shape is None else shape
        x1 = self.x[..., :self.C1].reshape(self.B, *shape, self.C1).contiguous().to("cuda", self.dtype)
        x2 = self.x[..., self.C1:].reshape(self.B, *shape, self.C2).contiguous().to("cuda", self.dtype) if self.C2 else None
        stats = ops.GNStats(self.st1.cuda(), self.st2.cuda() if self.C2 else None)
        return x1, x2, stats, self.gamma.cuda(), self.beta.cuda()


def _split_matrix(C2):
    return CONCAT_S if C2 else [(s, 0) for s in SINGLE_S]


# ------------------------------------------------------------------------------------------------ a. afldm_gn_stats, exact
HWS = [1, 3, 15, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
STATS_CASES = ([(hw, 64) for hw in HWS] + [(hw, c) for c in (4, 12) for hw in (1, 15, 65, 257, 1025)]
               + [(hw, c) for c in (1024, 2048, 8192) for hw in (3, 65)])


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("HW,C", STATS_CASES)
def test_gn_stats_exact(HW, C, dtype):
    """k_gn_partial per split against float64 sums of integer planes: every gn_splits band (1 / 4 / 16 / 32), HW % S != 0,
    splits shorter than one unrolled round of 4 ppl pixels; C = 4, 12 (ppl = 256, 85; idle threads), 64, 1024 (ppl = 1), 2048 (the
    strided channel-quad loop), 8192 (64 KB of LDS)."""
    ops = _ops()
    x = go.int_planes(B3, C, HW, HW + C, dtype)
    S = ops.lib.afldm_gn_stats_splits(HW)
    assert S == (32 if HW >= 1024 else 16 if HW >= 256 else 4 if HW >= 64 else 1)
    want = go.partials(x, go.even_cuts(HW, S))
    out = torch.full((B3, S, C, 2), float("nan"), dtype=torch.float32, device="cuda")
    xd = x.view(B3, HW, 1, C).to("cuda", dtype)
    st = ops.gn_stats(xd, out=out)
    assert st.st1 is out and st.st2 is None
    got = out.cpu()
    for s in range(S):
        assert torch.equal(got[:, s], want[:, s]), f"split {s} of {S} (pixels {HW * s // S}..{HW * (s + 1) // S})"


@pytest.mark.parametrize("C,msg", [(8196, "too wide"), (6, "multiple of 4")])
def test_gn_stats_refuses_on_the_host(C, msg):
    ops = _ops()
    x = torch.zeros(B3, 3, 1, C, device="cuda")
    out = torch.zeros(B3, 1, C, 2, device="cuda")
    with pytest.raises(RuntimeError, match=f"afldm_gn_stats: .*{msg}"):
        ops.gn_stats(x, out=out)


# ------------------------------------------------------------------------------------------------ b. afldm_gn_fold, exact
def _fold(st, S_out):
    from afldm_amd import _lib
    B, S_in, C, _ = st.shape
    out = torch.full((B, S_out, C, 2), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib.afldm_gn_fold(st.data_ptr(), S_in, out.data_ptr(), S_out, B, C, _lib.stream_ptr()), "gn_fold")
    return out


@pytest.mark.parametrize("C", [4, 192])
@pytest.mark.parametrize("S_in,S_out", [(512, 32), (8, 8), (9, 3), (6, 1)])
def test_gn_fold_exact(S_in, S_out, C):
    gen = torch.Generator().manual_seed(S_in + C)
    st = torch.randint(-4096, 4097, (B3, S_in, C, 2), generator=gen).float()          # 512 of them stay below 2^24
    want = st.double().view(B3, S_out, S_in // S_out, C, 2).sum(2).float()
    assert torch.equal(_fold(st.cuda(), S_out).cpu(), want)


def test_gn_fold_refuses_a_ragged_ratio():
    with pytest.raises(RuntimeError, match="afldm_gn_fold: S_in=9 must be a multiple of S_out=4"):
        _fold(torch.zeros(B3, 9, 8, 2, device="cuda"), 4)


# ------------------------------------------------------------------------------------------------ c. afldm_gn_apply
APPLY_SHAPES = [
    # C1, C2, G, HW, B, dtypes
    (12, 20, 8, 65, 3, DTYPES),          # bf16: C1 % 8 == 4 -> the non-streaming path; seam inside group 2; 65 rows
    (48, 0, 16, 15, 3, DTYPES),          # bf16: nc = 6, rl = 42 (4 idle threads); cpg = 3
    (96, 0, 48, 64, 3, DTYPES),          # G > 32: the second round of g0 += 32
    (64, 0, 64, 4, 3, DTYPES),           # cpg = 1
    (768, 384, 32, 5, 3, DTYPES),        # C > 1024: table_regs off; bf16 nc = 144
    (1028, 0, 4, 3, 3, [torch.float32]),   # C / EPC = 257 > 256 threads: non-streaming
    (2056, 0, 8, 3, 3, [BF16]),
    (64, 0, 32, 1, 3, DTYPES),           # HW = 1
    (64, 0, 32, 4096, 16, DTYPES),       # HW >= 4096 and a large tensor: 32768 elements per workgroup
]


def _check_apply(case, S1, S2, what):
    ops = _ops()
    x1, x2, stats, gamma, beta = case.dev()
    shape = (case.B, case.HW, 1, case.C)
    y0 = ops.gn_apply(x1, stats, gamma, beta, case.G, case.eps, act=0, x2=x2)
    y1 = ops.gn_apply(x1, stats, gamma, beta, case.G, case.eps, act=1, x2=x2)
    assert y0.shape == shape and y0.dtype == case.dtype
    got = y0.double().cpu().view(case.B, case.HW, case.C)
    assert torch.isfinite(got).all(), what
    frac = ((got - case.ref).abs() / go.apply_bound(case.x, case.k, case.sh, case.ref, case.dtype)).max().item()
    assert frac <= 1.0, f"{what} act=0: |err| / bound = {frac:.3f}"
    return y1, frac


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in APPLY_SHAPES for d in s[5]],
                         ids=lambda v: _id(v) if isinstance(v, torch.dtype) else "-".join(str(i) for i in v[:5]))
def test_gn_apply_splits(shape, dtype):
    """act = 0 inside the element-wise apply_bound (quiet and loud constant), act = 1 in the close() classes, over the split matrix
    and the three data variants.  The 4 M-element shape keeps to two split counts and one variant: its float64 side is what costs."""
    C1, C2, G, HW, B, _ = shape
    big = B * HW * (C1 + C2) > (1 << 20)
    worst = 0.0
    for ratio, starve, const in ([VARIANTS[2]] if big else VARIANTS + LOUD):
        case = None
        for S1, S2 in ([(9, 0), (32, 0)] if big else _split_matrix(C2)):
            if case is None:
                case = Case(B, C1, C2, G, HW, dtype, ratio, starve, const, S1, S2, seed=ratio)
            else:
                case.set_splits(S1, S2, starve, seed=ratio)
            what = f"gn_apply {shape[:5]} S=({S1},{S2}) ratio={ratio} starved={starve} const={const}"
            y1, frac = _check_apply(case, S1, S2, what)
            worst = max(worst, frac)
            if const != "loud":
                ref1 = torch.nn.functional.silu(case.ref)
                close(y1.float().cpu().view(B, HW, -1), ref1, dtype, what + " act=1", bf16_rms=4e-3)
    print(f"[gn_apply {shape[:5]} {_id(dtype)}] worst |err| / apply_bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ d. afldm_af_act and its forms
def _warped(ref, B, N, C):
    from oracle import ideal_filters as idf
    return idf.warped_nonlinearity(ref.view(B, N, N, C).permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


AF_SHAPES = [
    # N, C1, C2, G
    (2, 48, 96, 8),          # cpg = 18, seam inside group 2: gn_wave_keys, a wave spans 3 - 4 keys
    (2, 64, 0, 64),          # cpg = 1: 64 keys per wave, 16 rounds
    (4, 96, 48, 8),          # the VALU kernel (the default at N = 4; Kronecker MFMA: test_gpu_af_routes); cpg = 18, seam inside group 5
    (4, 36, 0, 6),           # C % 16 != 0: the VALU kernel; cpg = 6
    (8, 96, 48, 8),          # bf16: k_af_act_p8; fp32: Kronecker; cpg = 18
    (8, 64, 0, 32),          # cpg = 2
    (16, 16, 32, 8),         # plane kernel; cpg = 6, seam inside group 2; cpg * smax = 6 .. 192: both sides of 128
    (16, 64, 32, 4),         # cpg = 24, seam inside group 2; 24 * 4 = 96 (fast), 24 * 8 = 192 (in line)
    (16, 64, 0, 64),         # cpg = 1: an item (8 channels at B = 3) touches 8 groups (> 4 waves: `fast` / `n_piped` off)
    (16, 144, 0, 8),         # cpg = 18: an item touches 2 groups
    (32, 32, 16, 8),         # cpg = 6, seam inside group 5
    (32, 64, 0, 32),         # cpg = 2: 4 groups per 8-channel item (16-channel items, 8 groups: test_gpu_af_routes)
    (32, 192, 0, 8),         # cpg = 24
]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", AF_SHAPES, ids=lambda s: "-".join(str(v) for v in s) + ("-concat" if s[2] else ""))
def test_af_act_splits(shape, dtype):
    ops = _ops()
    N, C1, C2, G = shape
    C = C1 + C2
    for ratio, starve, const in VARIANTS:
        case = None
        for S1, S2 in _split_matrix(C2):
            if case is None:
                case = Case(B3, C1, C2, G, N * N, dtype, ratio, starve, const, S1, S2, seed=ratio + N)
                x1, x2, _, gamma, beta = case.dev((N, N))
            else:
                case.set_splits(S1, S2, starve, seed=ratio + N)
            stats = ops.GNStats(case.st1.cuda(), case.st2.cuda() if C2 else None)
            what = f"af_act {shape} S=({S1},{S2}) ratio={ratio} starved={starve}"
            ref = _warped(case.ref, B3, N, C)
            y = ops.af_act(x1, x2, stats, gamma, beta, G, case.eps)
            close(y.float().cpu(), ref, dtype, what)
            if N == 2:                                         # the plane-constant form: one value per plane
                yc = ops.af_act(x1, x2, stats, gamma, beta, G, case.eps, out_const=True)
                assert yc.shape == (B3, C)
                close(yc.float().cpu()[:, None, None, :].expand(B3, 2, 2, C), ref, dtype, what + " const2")
            if N >= 16 and dtype == BF16:                      # 8-channel blocks out, and in (a blocked input is one tensor)
                from test_gpu_r05 import _c8_to_nhwc, _nhwc_to_c8
                y8 = ops.af_act(x1, x2, stats, gamma, beta, G, case.eps, out_c8=True)
                assert ops.is_c8(y8) and torch.equal(_c8_to_nhwc(y8), y), what + " c8 out"
                if not C2:
                    y88 = ops.af_act(_nhwc_to_c8(x1), None, stats, gamma, beta, G, case.eps, out_c8=True)
                    assert torch.equal(_c8_to_nhwc(y88), y), what + " c8 in, c8 out"


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_af_act_pipelined_statistics_on_a_concat_with_unequal_splits(dtype):
    """As test_af_act_plane_pipelined_statistics_match_the_inline_path, on hard statistics: N = 16, 192 | 192 with (S1, S2) =
    (9, 4) at batch 64, where a workgroup walks several items (the pipelined copy of the group sums); two-sample sub-batches
    (first two items at once / in line) must agree bit for bit, and three samples with the oracle."""
    ops = _ops()
    N, C1, C2, G, B = 16, 192, 192, 32, 64
    case = Case(B, C1, C2, G, N * N, dtype, 32, True, 0.25, 9, 4, seed=3)
    x1, x2, stats, gamma, beta = case.dev((N, N))
    y = ops.af_act(x1, x2, stats, gamma, beta, G, case.eps)
    for b0 in (0, 31, 62):
        sub = ops.GNStats(stats.st1[b0:b0 + 2].contiguous(), stats.st2[b0:b0 + 2].contiguous())
        y2 = ops.af_act(x1[b0:b0 + 2].contiguous(), x2[b0:b0 + 2].contiguous(), sub, gamma, beta, G, case.eps)
        assert torch.equal(y2, y[b0:b0 + 2]), b0
    for b0 in (0, B // 2 - 1, B - 3):                          # B // 2 is the constant (starved) sample
        ref = _warped(case.ref[b0:b0 + 3], 3, N, C1 + C2)
        close(y[b0:b0 + 3].float().cpu(), ref, dtype, f"pipelined gn+af_act samples {b0}..{b0 + 2}")


# ------------------------------------------------------------------------------------------------ e. afldm_gn_table
@pytest.mark.parametrize("C,G", [(64, 32), (64, 64), (48, 16)])
def test_gn_table_splits(C, G):
    ops = _ops()
    HW = 64
    u = go.EPS24
    for ratio, starve, const in VARIANTS + LOUD:
        for S, _ in _split_matrix(0):
            case = Case(B3, C, 0, G, HW, torch.float32, ratio, starve, const, S, 0, seed=ratio)
            got = ops.gn_table(ops.GNStats(case.st1.cuda()), case.gamma.cuda(), case.beta.cuda(), B3, C, G, HW, case.eps).double().cpu()
            assert got.shape == (B3, C, 2) and torch.isfinite(got).all()
            mk = (case.beta.double() - case.sh).abs()                                  # |mean k|
            dk = ((got[..., 0] - case.k).abs() / case.k.abs()).max().item()
            dsh = ((got[..., 1] - case.sh).abs() / (mk + case.beta.double().abs())).max().item()
            what = f"gn_table C={C} G={G} S={S} ratio={ratio} starved={starve} const={const}"
            assert dk <= 4 * u, f"{what}: scale off by {dk / u:.2f} u"
            assert dsh <= 4 * u, f"{what}: shift off by {dsh / u:.2f} u"


# ------------------------------------------------------------------------------------------------ f. fused consumers
def _rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-30))


def test_conv_out_fused_splits():
    """afldm_conv_out_fused (gn_channel_sums, 8 lanes per group) against gn_apply (checked above) + conv2d on the same partials,
    in the tolerance test_unet_tail_norm_silu_conv_out_in_one_launch uses for that comparison (6e-3 rel-RMS)."""
    ops = _ops()
    B, N, C, Cout, G = 3, 32, 64, 3, 32
    gen = torch.Generator().manual_seed(5)
    w = ops.pack_weight((torch.randn(Cout, C, 3, 3, generator=gen) / (3 * C ** 0.5)).cuda(), BF16)
    bias = torch.randn(Cout, generator=gen).cuda()
    for ratio, starve, const in VARIANTS:
        for S, _ in _split_matrix(0):
            case = Case(B, C, 0, G, N * N, BF16, ratio, starve, const, S, 0, seed=ratio)
            x, _, stats, gamma, beta = case.dev((N, N))
            x.gn_partial = stats.st1                           # the op takes them from the tensor
            y = ops.conv_out_fused(x, w, bias, gamma, beta, G, case.eps)
            assert y is not None and y.shape == (B, N, N, Cout)
            plain = ops.conv2d(ops.gn_apply(x, stats, gamma, beta, G, case.eps, act=1), w, bias)
            d = _rel_rms(y, plain)
            assert torch.isfinite(y).all() and d <= 6e-3, f"conv_out_fused S={S} ratio={ratio} starved={starve}: {d:.3e}"


def test_attn_block_fused_splits():
    """afldm_attn_block_fused (its own quarter-wave walk over cpg x S partials, SV in flight) against gn_apply + linear_split +
    attention on the same partials, in the tolerance test_attn_block_fused_with_both_loops_live_in_one_workgroup uses (2e-2)."""
    ops = _ops()
    B, T, C, heads, G = 2, 256, 64, 4, 32
    assert ops.lib.afldm_attn_block_fused_supported(T, C, C // heads, G)
    gen = torch.Generator().manual_seed(6)
    w = ops.pack_weight((torch.randn(3 * C, C, generator=gen) / C ** 0.5).cuda(), BF16)
    bias = (0.1 * torch.randn(3 * C, generator=gen)).cuda()
    scale = (C // heads) ** -0.5
    for ratio, starve, const in VARIANTS:
        for S, _ in _split_matrix(0):
            case = Case(B, C, 0, G, T, BF16, ratio, starve, const, S, 0, seed=ratio)
            x, _, stats, gamma, beta = case.dev((16, 16))
            xt = x.view(B, T, C)
            got = ops.attn_block_fused(xt, stats, gamma, beta, G, case.eps, w, bias, heads, scale)
            hn = ops.gn_apply(x, stats, gamma, beta, G, case.eps, act=0).view(B, T, C)
            qk, vt = ops.linear_split(hn, w, bias, 2 * C)
            old = ops.attention(qk[:, :, :C], qk[:, :, C:], vt, heads, scale=scale)
            d = _rel_rms(got, old)
            assert torch.isfinite(got).all() and d <= 2e-2, f"attn_block_fused S={S} ratio={ratio} starved={starve}: {d:.3e}"


@pytest.mark.parametrize("B,T,C", [(3, 4, 64), (2, 16, 128)])
def test_attn_identity_block_splits(B, T, C, monkeypatch):
    """afldm_attn_identity_block against float64 from the same partials, in test_identity_block_against_float64's bound
    (2^-8 (A + |y|) + K 2^-24 A), and the two-launch composition on the gn_apply checked above inside the same bound."""
    ops = _ops()
    G = 32
    monkeypatch.setattr(ops, "_IDENTITY_MIN_T", 4)
    gen = torch.Generator().manual_seed(7)
    w = ops.pack_weight((torch.randn(C, C, generator=gen) / C ** 0.5).cuda(), BF16)
    bias = (0.1 * torch.randn(C, generator=gen)).cuda()
    wd = w.double().cpu().view(C, C)
    for ratio, starve, const in VARIANTS:
        for S, _ in _split_matrix(0):
            case = Case(B, C, 0, G, T, BF16, ratio, starve, const, S, 0, seed=ratio)
            x, _, stats, gamma, beta = case.dev((T,))
            assert ops.attn_identity_block_ok(x, G)
            got = ops.attn_identity_block(x, stats, gamma, beta, G, case.eps, w, bias)
            comp = ops.conv2d(ops.gn_apply(x, stats, gamma, beta, G, case.eps, act=0), w, bias, residual=x)
            y = case.x.double() + case.ref @ wd.T + bias.double().cpu()
            A = case.ref.abs() @ wd.abs().T
            tol = 2.0 ** -8 * (A + y.abs()) + C * 2.0 ** -24 * A
            for name, t in (("one launch", got), ("gn_apply + conv2d", comp)):
                r = float(((t.double().cpu() - y).abs() / tol).max())
                assert r <= 1.0, f"identity block ({name}) S={S} ratio={ratio} starved={starve}: error / bound {r:.3f}"


def test_act_conv_act_pre_splits():
    """afldm_act_conv_act with `pre` on a 384 | 192 concat (cpg = 18, seam inside group 21): its activated input is af_act on
    the same statistics, bit for bit (the copies of gn_group_sums_wave in actconv.hip), and the convolution behind it is
    conv2d of that tensor.  The merged kernel embeds the 128-pixel x 192-cout halo-patch tile (variant 43 at 16^2), which the
    convolution plan picks from 192 tiles on (batch 48 here); at batch 16 it is selected with afldm_conv2d_tune, for the merged
    launch and for the separate convolution alike, so that the small case runs the kernel under test and cannot fall back."""
    from afldm_amd import _exp, _lib
    if not _exp.available():
        pytest.skip("the experimental library (merged launches) is not built")
    ops = _ops()
    N, C1, C2, B, G, Cout = 16, 384, 192, 16, 32, 384
    gen = torch.Generator().manual_seed(8)
    w = ops.pack_weight((torch.randn(Cout, C1 + C2, 3, 3, generator=gen) * (9 * (C1 + C2)) ** -0.5).cuda(), BF16)
    bias = torch.randn(Cout, generator=gen).cuda()
    _lib.check(_lib.lib.afldm_conv2d_tune(43, 1), "tune")
    try:
        for ratio, starve, const in VARIANTS:
            case = None
            for S1, S2 in CONCAT_S:
                if case is None:
                    case = Case(B, C1, C2, G, N * N, BF16, ratio, starve, const, S1, S2, seed=ratio, eps=1e-6)
                    x1, x2, _, gamma, beta = case.dev((N, N))
                else:
                    case.set_splits(S1, S2, starve, seed=ratio)
                stats = ops.GNStats(case.st1.cuda(), case.st2.cuda())
                got = ops.act_conv_act(x1, x2, (stats, gamma, beta, G, case.eps), w, bias, want_stats=True)
                assert got is not None, "no merged kernel for the 16^2 level's up-block shape"
                a_ref = ops.af_act(x1, x2, stats, gamma, beta, G, case.eps)
                what = f"act_conv_act S=({S1},{S2}) ratio={ratio} starved={starve}"
                assert torch.equal(got[0].act_input, a_ref), what
                y_ref = ops.conv2d(a_ref, w, bias, want_stats=True)
                assert torch.equal(got[0], y_ref) and torch.equal(got[0].gn_partial, y_ref.gn_partial), what
            b0 = B // 2 - 1                                    # the three samples around the constant one
            close(a_ref[b0:b0 + 3].float().cpu(), _warped(case.ref[b0:b0 + 3], 3, N, C1 + C2), BF16, f"act_conv_act input ratio={ratio}")
    finally:
        _lib.lib.afldm_conv2d_tune(-1, -1)
    assert ops.actconv_error() == 0


# ------------------------------------------------------------------------------------------------ g. end to end, ratio <= 8
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("N,C1,C2,G", [(16, 64, 32, 4), (8, 96, 48, 8), (32, 64, 0, 32), (2, 48, 96, 8)])
def test_gn_stats_to_consumers_against_true_groupnorm(N, C1, C2, G, dtype):
    """afldm_gn_stats -> afldm_gn_apply / afldm_af_act on hard planes at ratio 8 against GroupNorm computed from the data itself
    in float64: the format's own rstd error (<= 2e-6 here, test_gn_oracle_host) is far inside the close() classes."""
    ops = _ops()
    C, HW = C1 + C2, N * N
    for ratio in (0.5, 8):
        x = go.hard_planes(B3, C, G, HW, ratio, N + C, dtype)
        gamma, beta = _affine(C, N)
        ref = go.true_groupnorm(x, gamma, beta, G, EPS)
        x1 = x[..., :C1].reshape(B3, N, N, C1).contiguous().to("cuda", dtype)
        x2 = x[..., C1:].reshape(B3, N, N, C2).contiguous().to("cuda", dtype) if C2 else None
        stats = ops.gn_stats(x1, G, x2=x2)
        assert stats.S1 == ops.lib.afldm_gn_stats_splits(HW)
        for act in (0, 1):
            y = ops.gn_apply(x1, stats, gamma.cuda(), beta.cuda(), G, EPS, act=act, x2=x2)
            want = torch.nn.functional.silu(ref) if act else ref
            close(y.float().cpu().view(B3, HW, C), want, dtype, f"gn_stats -> gn_apply act={act} ratio={ratio}", bf16_rms=4e-3)
        y = ops.af_act(x1, x2, stats, gamma.cuda(), beta.cuda(), G, EPS)
        close(y.float().cpu(), _warped(ref, B3, N, C), dtype, f"gn_stats -> af_act ratio={ratio}")


# ------------------------------------------------------------------------------------------------ h. ops without a test so far
def test_carry_stats_hands_the_partials_to_a_view():
    ops = _ops()
    x = torch.randn(2, 4, 4, 8, device="cuda")
    st = ops.gn_stats(x).st1
    v = ops.carry_stats(x.view(2, 16, 1, 8), x)
    assert v.gn_partial is st and ops.gn_stats(v).st1 is st                # no second pass
    bare = torch.randn(2, 4, 4, 8, device="cuda")
    assert getattr(ops.carry_stats(bare.view(2, 16, 1, 8), bare), "gn_partial", None) is None


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_af_resample_hw_against_float64(dtype):
    """y = Mh x Mw^T per plane with different matrices along H and W (the smallest shape: 4 x 4 -> 6 x 6, 4 channels)."""
    ops = _ops()
    gen = torch.Generator().manual_seed(4)
    B, N, R, C = 2, 4, 6, 4
    x = torch.randn(B, N, N, C, generator=gen).to(dtype)
    Mh, Mw = torch.randn(R, N, generator=gen), torch.randn(R, N, generator=gen)
    y = ops.af_resample_hw(x.cuda(), Mh.cuda(), Mw.cuda())
    ref = torch.einsum("rh,bhwc,sw->brsc", Mh.double(), x.double(), Mw.double())
    close(y.float().cpu(), ref, dtype, "af_resample_hw", bf16_rms=4e-3)
    same = ops.af_resample(x.cuda(), Mh.cuda())
    assert torch.equal(ops.af_resample_hw(x.cuda(), Mh.cuda(), Mh.cuda()), same)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_masked_metrics_against_float64(dtype):
    """[B, 6] = (sum ((a - b) m)^2, sum m, max a m, min a m, max b m, min b m) per sample; a broadcast mask counts a pixel once."""
    ops = _ops()
    gen = torch.Generator().manual_seed(9)
    B, C, H, W = 3, 2, 4, 5
    a = torch.randn(B, C, H, W, generator=gen).to(dtype)
    b = (a.float() + 0.3 * torch.randn(B, C, H, W, generator=gen)).to(dtype)
    for mask in ((torch.rand(B, C, H, W, generator=gen) > 0.4).float(), (torch.rand(B, 1, H, W, generator=gen) > 0.4).float()):
        got = ops.masked_metrics(a.cuda(), b.cuda(), mask.cuda()).double().cpu()
        ad, bd, m = a.double(), b.double(), mask.double().expand(B, C, H, W)
        am, bm = (ad * m).flatten(1), (bd * m).flatten(1)
        want = torch.stack([((ad - bd) * m).pow(2).flatten(1).sum(1), mask.double().flatten(1).sum(1), am.max(1).values,
                            am.min(1).values, bm.max(1).values, bm.min(1).values], 1)
        # 40 terms summed in fp32 (n 2^-24 relative, the recursive-summation bound); the extrema are values of the inputs
        assert ((got[:, 0] - want[:, 0]).abs() <= 40 * go.EPS24 * want[:, 0]).all(), (got[:, 0], want[:, 0])
        assert torch.equal(got[:, 1:], want[:, 1:]), (got, want)
