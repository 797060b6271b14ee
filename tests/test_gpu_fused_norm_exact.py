"""GPU tests: the launches that normalise a convolution's own output - afldm_conv2x2_const_norm_act (dense2.hip), afldm_af_act_slabs
(k_af_act_slabs, af.hip) and the y_norm epilogue of the one-sample 8x8 halo tile (conv3h_body.inc, variant 51) - element by element
against plain float64 on integer planes (tests/fusednorm_oracle.py; the CPU side is tests/test_fusednorm_oracle_host.py).

The producer's operands are small integers, so the value it stores and normalises is exact, the group sums are exact integers and
(mean, variance) do not depend on the summation order.  Every element of a normalised / activated output is then held to
2^-8 |ref| + 2^-16 max|hn| in bf16 (the half-ulp of the one store + the fp32 arithmetic in front of it) and to 2e-5 max|ref| in fp32;
raw outputs (want_raw, y) and the statistics must be EQUAL.  A lost K step of one wave's slice, a plane's pixels in another order,
a neighbouring sample's time-embedding row, statistics over 3 of 4 tiles and gamma / beta read one channel off each leave that
tolerance (planted on the CPU in the host file); the whole-tensor rel-RMS bounds of the older tests see none of them in one tile.

Sibling launches on the same integer inputs (fused dense2 against conv2d + af_act(out_const); af_act_slabs(act = 0) against the
reduction launch + gn_apply; y_norm against gn_apply of y with y's own partials) are held to the same float64 tolerance and are
bit-identical to the fused launch on every case (torch.equal).  Every test prints its worst error / tolerance.
"""
import pytest
import torch

import fusednorm_oracle as fo
from exact_oracle import assert_exact, assert_stats_exact

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = [FP32, BF16]

# the classes these cases run, for the coverage guard of the host file: (dtype, cpg, K steps per wave), (N, cpg, nslab) - run in both
# dtypes - and the y_norm cpg (bf16)
DENSE2_CLASSES = {(dt, Cout // G, fo.dense2_cin(steps, dt) // (fo.D2_WAVES * fo.kpf(dt)))
                  for dt in DTYPES for (_, steps, Cout, G, _, _, _) in fo.DENSE2_CASES}
SLAB_CLASSES = {(N, C // G, nslab) for (nslab, N, _, C, G, _, _, _, _) in fo.SLAB_CASES}
YNORM_CLASSES = {Cout // G for (_, _, Cout, G, _, _) in fo.YNORM_CASES}


def _ops():
    from afldm_amd import ops
    return ops


def dev(t, dtype):
    return None if t is None else t.to(dtype).cuda().contiguous()


def temb_dev(c, dtype):
    """The case's time embedding as the kernel is handed it: "wide" is a column slice of a wider row (temb_stride > C)."""
    if c.temb_full is None:
        return None
    full = dev(c.temb_full, dtype)
    return full if c.temb_mode != "wide" else full[:, c.temb_col0:c.temb_col0 + c.C]


def sibling(kind, a, b, what):
    """The fused launch and the launches it replaces gave the same bits on every case of the first MI355X run (same operation order,
    same gn_mean_rstd finish, exact sums): that is the assertion."""
    assert torch.equal(a, b), f"{what}: the {kind} launch and its sibling differ in {int((a != b).sum())} elements"


# ================================================================================================ a. af_act_slabs on dictated slabs
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("i", range(len(fo.SLAB_CASES)))
def test_af_act_slabs_on_dictated_slabs(dtype, i):
    """nslab 1 ... 9 (the unrolled first four and the rolled rest), N = 2 / 4, act 0 / 1 / 2, workgroups of 48 ... 256 threads, every
    temb form, residual, want_raw (bit for bit) and bias = None: fusednorm_oracle.SLAB_CASES, B = 3."""
    ops = _ops()
    c = fo.slab_case(*fo.SLAB_CASES[i])
    out = ops.af_act_slabs(c.slabs.cuda(), c.nslab, dev(c.bias, FP32), temb_dev(c, dtype), c.temb_stride, c.gamma.cuda(), c.beta.cuda(),
                           c.G, c.eps, c.B, c.N, c.C, dtype, residual=dev(c.residual, dtype), want_raw=c.want_raw,
                           act={0: False, 1: True, 2: 2}[c.act])
    if c.want_raw:
        out, raw = out
        assert_exact(raw.reshape(c.y.shape), c.y, c.what + " raw")
    assert out.shape == ((c.B, c.C) if c.act == 2 else (c.B, c.N, c.N, c.C))
    worst = fo.check_elements(out, c.ref, c.hn, dtype, c.what)
    print(f"[fusednorm] slabs {c.what} {dtype}: error / tolerance {worst:.3f}")


# ================================================================================================ b. conv2x2_const_norm_act
def _dense2_weights(c, dtype):
    """w_cm [4 Cout, 1, 1, Cin] on the GPU: through the model's packer from a ternary nn.Conv2d (which must give the float64 tap
    sums bit for bit) or dictated directly."""
    if c.conv_w is None:
        return dev(c.w_cm.view(4 * c.Cout, 1, 1, c.Cin), dtype)
    from afldm_amd.models import blocks
    conv = torch.nn.Conv2d(c.Cin, c.Cout, 3, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(c.conv_w)
    w = blocks.packed_conv_dense2x2_const_cm(conv.cuda(), dtype)
    assert_exact(w.reshape(4 * c.Cout, c.Cin), fo.tap_sum_cm(c.conv_w), c.what + " packed tap sums")
    return w


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("i", range(len(fo.DENSE2_CASES)))
def test_conv2x2_const_norm_act_on_integer_planes(dtype, i):
    """K steps per wave 1, 2, 3, 4, 6, 7, 13 (12 at the model's 1536 -> 768 in fp32), 8 / 12 / 24 channels per group (NT = 2 / 3 / 6),
    B = 1, 16, 17, 33, every temb form, bias = None, both weight recipes: fusednorm_oracle.DENSE2_CASES.  The sibling - conv2d on the
    same tap sums, then af_act(out_const) - stores the convolution (exact) and is held to the same tolerance."""
    ops = _ops()
    from afldm_amd.models import blocks
    c = fo.dense2_case(*fo.DENSE2_CASES[i], dtype)
    assert ops.conv2x2_const_norm_act_ok(c.Cin, c.Cout, c.G, dtype), c.what
    a, w, bias, temb = dev(c.a, dtype), _dense2_weights(c, dtype), dev(c.bias, FP32), temb_dev(c, dtype)
    gamma, beta = c.gamma.cuda(), c.beta.cuda()
    got = ops.conv2x2_const_norm_act(a, w, bias, temb, c.temb_stride, gamma, beta, c.G, c.eps)
    assert got.shape == (c.B, c.Cout)
    worst = fo.check_elements(got, c.ref, c.hn, dtype, c.what)
    # the launches it replaces: rows pixel-major (row = pixel * Cout + n), bias per row
    w_pm = w.view(c.Cout, 4, c.Cin).permute(1, 0, 2).reshape(4 * c.Cout, 1, 1, c.Cin).contiguous()
    kw = {} if temb is None else dict(temb=temb, temb_stride=c.temb_stride, temb_mod=c.Cout)
    y = ops.conv2d(a, w_pm, None if bias is None else bias.repeat(4).contiguous(), want_stats=True, **kw)
    assert_exact(y.view(c.B, 4, c.Cout), c.y, c.what + " conv2d")
    y4 = blocks._plane2_view(y, c.B, c.Cout)
    sib = ops.af_act(y4, None, ops.gn_stats(y4, c.G), gamma, beta, c.G, c.eps, out_const=True)
    w2 = fo.check_elements(sib, c.ref, c.hn, dtype, c.what + " (conv2d + af_act)")
    print(f"[fusednorm] dense2 {c.what} {dtype}: error / tolerance {worst:.3f} (sibling {w2:.3f})")
    sibling("dense2", got, sib, f"{c.what} {dtype}")


# ================================================================================================ c. conv2d_slabs -> af_act_slabs
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("i", range(len(fo.CHAIN_CASES)))
def test_conv2d_slabs_into_af_act_slabs(dtype, i):
    """A real split-K convolution's slabs (exact_oracle.conv_case with a density that keeps sigma <= 12) finished both ways: + bias +
    temb -> GroupNorm -> activation (conv1 -> norm2), and + bias + residual -> raw (bit for bit) and GroupNorm only (conv2 -> the
    attention block's norm); the last case carries the folded shortcut in its slabs.  The batch-64 plans must split K; a smaller
    batch whose plan does not is skipped with that reason.  Sibling: the same convolution with its reduction launch, then gn_apply."""
    ops = _ops()
    B, N, Cin, Cout, scC = fo.CHAIN_CASES[i]
    c = fo.chain_case(B, N, Cin, Cout, scC)
    G, eps, P = fo.CHAIN_G, fo.EPS, N * N
    x, w, bias, temb, res = dev(c.x1, dtype), dev(c.w, dtype), dev(c.bias, FP32), dev(c.temb, dtype), dev(c.residual, dtype)
    sc = None if c.shortcut is None else tuple(dev(t, dtype) for t in c.shortcut)
    gamma, beta = c.gamma.cuda(), c.beta.cuda()
    if sc is not None:
        assert ops.conv2d_shortcut_ok(x, w, None, sc, slabs=True) == 2, c.what
    got = ops.conv2d_slabs(x, w, shortcut=sc)
    if got is None:
        assert B < 64, f"{c.what} {dtype}: the batch-64 plan does not split K"
        pytest.skip(f"{c.what} {dtype}: the plan does not split K")
    slabs, nslab = got
    assert nslab > 1
    assert_exact(slabs.double().sum(0).view(B, P, Cout), c.plain, f"{c.what}: sum of {nslab} slabs")
    y1, hn1, ref1 = c.fin["act"]
    out = ops.af_act_slabs(slabs, nslab, bias, temb, Cout, gamma, beta, G, eps, B, N, Cout, dtype, act=True)
    wa = fo.check_elements(out, ref1, hn1, dtype, c.what + " act")
    y2, hn2, _ = c.fin["norm"]
    hn, raw = ops.af_act_slabs(slabs, nslab, bias, None, 0, gamma, beta, G, eps, B, N, Cout, dtype, residual=res, want_raw=True, act=False)
    assert_exact(raw.view(B, P, Cout), y2, c.what + " raw")
    wn = fo.check_elements(hn, hn2, hn2, dtype, c.what + " norm")
    # the sibling: reduction launch, then gn_apply with the statistics the reduction attached
    two = ops.conv2d(x, w, bias, residual=res, want_stats=True, shortcut=sc)
    assert_exact(two.view(B, P, Cout), y2, c.what + " conv2d")
    assert_stats_exact(two.gn_partial, two, c.what + " conv2d")
    hn_two = ops.gn_apply(two, ops.gn_stats(two), gamma, beta, G, eps)
    ws = fo.check_elements(hn_two, hn2, hn2, dtype, c.what + " (reduction + gn_apply)")
    print(f"[fusednorm] chain {c.what} {dtype} nslab {nslab}: error / tolerance act {wa:.3f} norm {wn:.3f} (sibling {ws:.3f})")
    sibling("slabs", hn, hn_two, f"{c.what} {dtype}")


# ================================================================================================ d. the y_norm epilogue
@pytest.mark.parametrize("i", range(len(fo.YNORM_CASES)))
def test_y_norm_epilogue_on_integer_planes(i):
    """8^2 planes, bf16, the one-sample tile with the whole K per workgroup: y and its statistics exact, y.norm_applied within the
    tolerance, at the first batch afldm_conv2d_norm_ok accepts and at 64; 6 / 12 / 24 / 48 channels per group; with the folded
    shortcut.  Sibling: gn_apply of y with y's own partials."""
    ops = _ops()
    B, Cin, Cout, G, scC, has_temb = fo.YNORM_CASES[i]
    c = fo.ynorm_case(B, Cin, Cout, G, scC, has_temb)
    x, w, bias, temb = dev(c.x1, BF16), dev(c.w, BF16), dev(c.bias, FP32), dev(c.temb, BF16)
    sc = None if c.shortcut is None else tuple(dev(t, BF16) for t in c.shortcut)
    gamma, beta = c.gamma.cuda(), c.beta.cuda()
    kw = dict(temb=temb, temb_stride=0 if temb is None else Cout)
    if sc is not None:
        kw["shortcut"] = sc
    y = ops.conv2d(x, w, bias, want_stats=True, norm_out=(gamma, beta, G, fo.EPS), **kw)
    hn = getattr(y, "norm_applied", None)
    assert hn is not None, f"{c.what}: afldm_conv2d_norm_ok refused the case"
    assert_exact(y, c.ref, c.what + " y")
    assert_stats_exact(y.gn_partial, y, c.what)
    worst = fo.check_elements(hn, c.hn, c.hn, BF16, c.what + " y_norm")
    sib = ops.gn_apply(y, ops.gn_stats(y), gamma, beta, G, fo.EPS)
    w2 = fo.check_elements(sib, c.hn, c.hn, BF16, c.what + " (gn_apply)")
    print(f"[fusednorm] y_norm {c.what} G{G}: error / tolerance {worst:.3f} (sibling {w2:.3f})")
    sibling("ynorm", hn, sib, c.what)
