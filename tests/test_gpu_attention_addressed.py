"""GPU tests: the fused attention block (csrc/attnf.hip) element by element against float64 on addressed inputs.

tests/addressed_oracle.py builds tokens, GroupNorm partials and projections of small integers on which query i of head h returns
row pi_h(i) of v (a bijection per head that crosses the 32-token tiles), or the mean over all keys, or the mean over the T / 4
keys that share two code bits - so that a dropped key or tile, two swapped V rows, a row sum that misses a key, a rotated query
tile, another head's to_v rows or another sample's partials move the float64 reference by O(1) while no legitimate rounding moves
it at all.  Every element is held to tol = 2^-8 |ref| + 4 (1 - p_in) max|v| (derived there); tests/test_addressed_oracle_host.py
asserts the conditions behind it, plants those faults on the CPU and shows which attention loop every tile takes.

Every shape afldm_attn_block_fused_supported admits, B = 3, G = 32, the three recipes, partials in 1 and 9 ragged splits, bf16.
Every test prints the worst |got - ref| / tol it saw.  Measured on MI355X: addressed 3e-3 ... 1.1e-2 (the mass term where v is 0,
nothing elsewhere), uniform and subset up to 0.996 (the half-ulp of the bf16 store of a mean just above a power of two), the same
figures from the fused launch, with the row-maxima loop forced and from the three-launch path; attn_block_fused_out 3e-6 / 0.57 /
0.73 on y and at most 0.05 of the bound on the statistics."""
import os

import pytest
import torch

import addressed_oracle as ado

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, G = 3, 32
B_OUT, OUT_SHAPE = 8, (1024, 192, 8)
SHAPE_IDS = [f"T{T}-C{C}-h{h}" for T, C, h in ado.SHAPES]


def _ops():
    from afldm_amd import ops
    return ops


def _operands(c, S):
    """The case on the GPU: (x [B, T, C] bf16, GNStats of the fabricated partials, gamma, beta, packed to_q | to_k | to_v, bias)."""
    ops = _ops()
    x = c.x.to(BF16).cuda()
    stats = ops.GNStats(ado.partials(c.m, c.C, c.T, S, c.seed).cuda())
    w = ops.pack_weight(torch.cat([c.wq, c.wk, c.wv], 0).float().cuda(), BF16)
    bias = torch.cat([c.bq, c.bk, c.bv], 0).float().cuda()
    return x, stats, c.gamma.float().cuda(), c.beta.float().cuda(), w, bias


def _forced_row_maxima(fn):
    os.environ["AFLDM_ATTNF_SLOW"] = "1"
    try:
        return fn()
    finally:
        del os.environ["AFLDM_ATTNF_SLOW"]


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("recipe", ado.RECIPES)
@pytest.mark.parametrize("T,C,heads", ado.SHAPES, ids=SHAPE_IDS)
def test_attn_block_fused_addressed(T, C, heads, recipe, S):
    """ops.attn_block_fused per element against float64, as the kernel chooses its loops and once more with the row-maxima loop
    forced on every wave."""
    ops = _ops()
    c = ado.cached_attention_case(B, T, C, heads, recipe)
    assert ops.lib.afldm_attn_block_fused_supported(T, C, C // heads, G)
    x, stats, gamma, beta, w, bias = _operands(c, S)
    got = ops.attn_block_fused(x, stats, gamma, beta, G, ado.EPS, w, bias, heads, c.scale)
    slow = _forced_row_maxima(lambda: ops.attn_block_fused(x, stats, gamma, beta, G, ado.EPS, w, bias, heads, c.scale))
    torch.cuda.synchronize()
    r_got = ado.assert_addressed(got, c, f"attn_block_fused S={S}")
    r_slow = ado.assert_addressed(slow, c, f"attn_block_fused S={S}, row-maxima loop forced")
    print(f"[addressed] attn_block_fused {c.what} S={S}: worst error / tol {r_got:.3e}, row-maxima loop forced {r_slow:.3e}")


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("recipe", ado.RECIPES)
@pytest.mark.parametrize("T,C,heads", ado.SHAPES, ids=SHAPE_IDS)
def test_three_launch_path_addressed(T, C, heads, recipe, S):
    """The same cases through gn_apply -> linear_split -> attention, against the same tolerance: the case is sound on the device
    independently of attnf.hip (the normalised tokens and q | k | v are exact quantities on the way: asserted)."""
    ops = _ops()
    c = ado.cached_attention_case(B, T, C, heads, recipe)
    x, stats, gamma, beta, w, bias = _operands(c, S)
    side = int(T ** 0.5)
    hn = ops.gn_apply(x.view(B, side, side, C), stats, gamma, beta, G, ado.EPS, act=0).view(B, T, C)
    qk, vt = ops.linear_split(hn, w, bias, 2 * C)
    got = ops.attention(qk[:, :, :C], qk[:, :, C:], vt, heads, scale=c.scale)
    torch.cuda.synchronize()
    assert torch.equal(hn.double().cpu(), c.h), "gn_apply on the fabricated partials"
    assert torch.equal(vt.transpose(1, 2).double().cpu(), c.v), "to_v"
    r = ado.assert_addressed(got, c, f"three launches S={S}")
    print(f"[addressed] three launches {c.what} S={S}: worst error / tol {r:.3e}")


@pytest.mark.parametrize("recipe", ado.RECIPES)
def test_attn_block_fused_out_addressed(recipe):
    """ops.attn_block_fused_out at the one shape it has a kernel for, batch 8, inside a sync scope, with a ternary to_out and an
    integer bias: y = to_out(o) + x against float64 (one bf16 ulp of y plus the tolerance of o carried through the sum of
    |w_out|); gn_partial against float64 sums of the STORED y over each workgroup's 128-token block, relative to the sum of the
    magnitudes, within 128 * 2^-24 (an fp32 summation of 128 terms); hand-over counters and error word back at zero; reruns
    bit-identical.  Partials in 1 and 9 splits."""
    ops = _ops()
    T, C, heads = OUT_SHAPE
    c = ado.to_out_case(ado.cached_attention_case(B_OUT, T, C, heads, recipe))
    wo = ops.pack_weight(c.wo.float().cuda(), BF16)
    bo = c.bo.float().cuda()
    TB = T // heads
    for S in (1, 9):
        x, stats, gamma, beta, w, bias = _operands(c, S)
        assert ops.attn_block_fused_out_ok(x, heads, G)
        sync = ops.new_sync_buffer(x.device)
        with ops.sync_scope(sync):
            y = ops.attn_block_fused_out(x, stats, gamma, beta, G, ado.EPS, w, bias, heads, c.scale, wo, bo)
            y2 = ops.attn_block_fused_out(x, stats, gamma, beta, G, ado.EPS, w, bias, heads, c.scale, wo, bo)
        torch.cuda.synchronize()
        assert int(sync.abs().sum().item()) == 0, "hand-over counters / error word must be back at zero"
        assert torch.equal(y, y2) and torch.equal(y.gn_partial, y2.gn_partial), "reruns differ"
        r = ado.assert_addressed(y, c, f"attn_block_fused_out S={S}", ref=c.y, tol=c.y_tol)
        assert y.gn_partial.shape == (B_OUT, heads, C, 2)
        yd = y.double().cpu().view(B_OUT, heads, TB, C)
        direct = torch.stack([yd.sum(2), (yd * yd).sum(2)], -1)
        scale = torch.stack([yd.abs().sum(2), (yd * yd).sum(2)], -1)
        err = (y.gn_partial.double().cpu() - direct).abs()
        bound = TB * 2.0 ** -24 * scale
        worst = float((err / bound.clamp_min(1e-300))[bound > 0].max())
        print(f"[addressed] attn_block_fused_out {c.what} S={S}: worst y error / tol {r:.3e}, statistics error / bound {worst:.3e}")
        assert bool((err <= bound).all()), f"statistics S={S}: {int((err > bound).sum())} partial sums outside {TB} * 2^-24 of the stored y"
        if c.y_int is not None:           # the addressed recipe: y is an exact quantity wherever it is not zero
            nz = c.y_int != 0
            assert torch.equal(y.double().cpu()[nz], c.y_int[nz])
