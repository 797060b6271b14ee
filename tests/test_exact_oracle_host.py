"""CPU checks of tests/exact_oracle.py: every case of the GPU file's tables meets the two caps on the reference alone, each
planted mutation of a restated convolution is caught by assert_exact, and the loose bf16 bound of tests/test_gpu_ops.py misses
the three localised ones on Gaussian data - the gap that tests/test_gpu_exact_gemm.py closes."""
import pytest
import torch

import addressed_oracle as ado
import exact_oracle as xo
from test_gpu_ops import close


@pytest.mark.parametrize("name,thunk", xo.static_cases(), ids=[n for n, _ in xo.static_cases()])
def test_case_tables_meet_the_caps(name, thunk):
    """conv_case asserts max|y| <= 256 and sum(y^2) < 2^24 per (sample, channel) itself; operands and reference survive the
    fp32 and bf16 roundings unchanged."""
    c = thunk()
    assert c.max_abs <= xo.MAX_ABS and c.max_sumsq < xo.MAX_SUMSQ
    for dtype in (torch.float32, torch.bfloat16):
        assert xo.operands_survive(c, dtype), (name, dtype)


def test_caps_are_conditions():
    """A case that breaks a cap is refused (every weight non-zero at K = 55296: sigma(y) is about 140)."""
    with pytest.raises(AssertionError, match="bad case"):
        xo.conv_case(1, 4, 4, 3072, 3072, 64, w_density=1.0)


def test_helpers():
    g = torch.Generator().manual_seed(1)
    t = xo.ternary((4000,), 0.25, g)
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0} and 0.2 < float((t != 0).float().mean()) < 0.3
    s = xo.small_ints((4000,), -8, 8, g)
    assert float(s.min()) == -8 and float(s.max()) == 8 and torch.equal(s, s.round())
    c = xo.conv_case(2, 4, 4, 64, 0, 64, temb=True, residual=True)
    xo.assert_exact(c.ref.to(torch.bfloat16), c.ref, "round trip")
    st = torch.stack([c.ref.sum((1, 2)), (c.ref * c.ref).sum((1, 2))], -1).float()            # one split
    xo.assert_stats_exact(torch.stack([st * 0.25, st * 0.75], 1), c.ref.float(), "two splits")
    with pytest.raises(AssertionError, match=r"sum\(y\^2\)"):
        xo.assert_stats_exact(torch.stack([st, st * 0 + torch.tensor([0.0, 1.0])], 1), c.ref.float())
    bad = c.ref.clone()
    bad[1, 3, 0, 5] += 1
    with pytest.raises(AssertionError, match=r"1 of 2048 values differ.*\(1, 3, 0, 5\)"):
        xo.assert_exact(bad, c.ref, "one value")


# ------------------------------------------------------------------------------------------------ the fused UNet tail
TAIL_CASES = [(C, Cout, G) for C in (64, 128, 192) for Cout, G in ado.tail_grid(C)]


def test_silu_on_the_allowed_set():
    """torch's fp32 SiLU rounded to bf16 returns v on {0, 8, 16, 24, 32} (silu moves v by a relative e^-v <= 3.4e-4, under the
    2^-9 half-ulp) and zero on {-128, -256} (sigmoid underflows) - with an ulp of fp32 either way on v, too."""
    v = torch.tensor(ado.TAIL_IDENTITY + ado.TAIL_ZERO, dtype=torch.float32)
    want = ado.expected_silu_bf16(v.double())
    for t in (v, torch.nextafter(v, v + 1), torch.nextafter(v, v - 1)):
        got = torch.nn.functional.silu(t).to(torch.bfloat16).double()
        ok = (got == want) | ((want == 0) & (got.abs() <= 1e-6))          # (an ulp beside 0 is not 0: silu(x) ~ x / 2 there)
        assert bool(ok.all()), (t.tolist(), got.tolist())
    assert torch.equal(torch.nn.functional.silu(v).to(torch.bfloat16).double(), want)


@pytest.mark.parametrize("C,Cout,G", TAIL_CASES)
def test_tail_cases_meet_the_caps(C, Cout, G):
    """tail_case asserts the allowed set on the normalised values and integral y / 8 with |y / 8| <= 256 and sum((y / 8)^2) < 2^24
    itself; the operands survive bf16, and the partials of every split count finish to (m, 1) (partials asserts it)."""
    c = ado.tail_case(ado.TAIL_B, C, Cout, G)
    assert c.max_abs <= xo.MAX_ABS and c.max_sumsq < xo.MAX_SUMSQ
    for t in (c.x, c.w.double(), c.gamma, c.beta, c.ref):
        assert ado.is_bf16(t)
    assert torch.equal(c.bias, (c.bias / 8).round() * 8) and float(c.bias.abs().max()) <= 64
    live = set(c.norm.unique().tolist())
    assert live & set(ado.TAIL_ZERO) and live >= set(ado.TAIL_IDENTITY), f"the case does not reach both branches of silu: {sorted(live)}"
    for S in ado.SPLITS:
        ado.partials(c.m, C, c.N * c.N, S, c.seed)


def test_tail_oracle_catches_planted_faults():
    """A kernel that normalised and activated its zero padding (the shift beta - m gamma of sample 0 in every padded position), one
    that took the statistics of the neighbouring sample, and one that lost the last input channel of one tap: each is caught by
    assert_exact; the first differs on border pixels only."""
    c = ado.tail_case(ado.TAIL_B, 192, 3, 32)
    xo.assert_exact(ado.tail_reference(c.act, c.w, c.bias).to(torch.bfloat16), c.ref, "round trip")
    cpg = c.C // c.G
    pad = ado.expected_silu_bf16(c.beta)                                       # GroupNorm of a raw 0 with m = 0: beta
    bad = ado.tail_reference(c.act, c.w, c.bias, activate_padding=pad)
    diff = bad != c.ref
    assert bool(diff.any()) and not bool(diff[:, 1:-1, 1:-1].any())
    assert float((bad - c.ref).abs()[diff].min()) >= 8
    with pytest.raises(AssertionError, match="differ from the float64 reference"):
        xo.assert_exact(bad.to(torch.bfloat16), c.ref, "activated padding")
    m_wrong = c.m.roll(1, 0).repeat_interleave(cpg, 1)[:, None, None, :]
    act = torch.nn.functional.silu(c.gamma * (c.x - m_wrong) + c.beta).to(torch.bfloat16).double()     # (values off the allowed set)
    with pytest.raises(AssertionError, match="differ from the float64 reference"):
        xo.assert_exact(ado.tail_reference(act, c.w, c.bias).to(torch.bfloat16), c.ref, "another sample's statistics")
    w = c.w.clone()
    live = (w[:, 2, 2, :] != 0).any(0).nonzero()[-1]
    w[:, 2, 2, int(live)] = 0
    with pytest.raises(AssertionError, match="differ from the float64 reference"):
        xo.assert_exact(ado.tail_reference(c.act, w, c.bias).to(torch.bfloat16), c.ref, "a dropped tap channel")


# ------------------------------------------------------------------------------------------------ planted mutations
# The model's widest reduction: 768 | 768 -> 768 at 4^2 (K = 13824), eight samples with a time embedding.
SHAPE = dict(B=8, N=4, C1=768, C2=768, Cout=768)
TILE_N = 48            # couts of one workgroup's tile at this site (the 128-pixel x 48-cout halo tiles): a fault of one tile's waves stays inside it
KBLOCK = 64            # channels of one K step (128 bytes of bf16): the halo patch is staged once per channel block
MUTATIONS = ["drop_tap_channel", "halo_corner", "seam_channel", "drop_last_row", "temb_row"]
LOCALISED = MUTATIONS[:3]


def restated_conv(x1, x2, w, bias, temb, mutation=None):
    """conv3x3 'same' of the virtual concat x1 | x2 (NHWC, OHWI weights) + bias + per-sample time embedding in float64, as nine
    shifted GEMMs over a zero-padded halo - with one fault planted:
      drop_tap_channel: the last input channel of tap (2, 2) is not accumulated;
      halo_corner:      output pixel (1, 1) of sample 0 reads zeros for its top-left halo pixel (0, 0) in the last channel block;
      seam_channel:     in the first cout tile, the first channel of x2 is read from x1 (its last channel) instead;
      drop_last_row:    the last output row (pixel) of the last sample is never written;
      temb_row:         sample 1 gets the time-embedding row of sample 0."""
    B, N, _, C1 = x1.shape
    Cout = w.shape[0]
    x = torch.cat([x1, x2], -1).double()
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    wd = w.double()
    y = torch.zeros(B, N, N, Cout, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            wt = wd[:, kh, kw, :]
            if mutation == "drop_tap_channel" and (kh, kw) == (2, 2):
                wt = wt.clone()
                wt[:, -1] = 0
            y += xp[:, kh:kh + N, kw:kw + N, :] @ wt.t()
    if mutation == "halo_corner":
        y[0, 1, 1] -= x[0, 0, 0, -KBLOCK:] @ wd[:, 0, 0, -KBLOCK:].t()
    if mutation == "seam_channel":
        xm = x.clone()
        xm[..., C1] = x[..., C1 - 1]
        xmp = torch.nn.functional.pad(xm, (0, 0, 1, 1, 1, 1))
        ym = sum(xmp[:, kh:kh + N, kw:kw + N, :] @ wd[:TILE_N, kh, kw, :].t() for kh in range(3) for kw in range(3))
        y[..., :TILE_N] = ym
    y = y + bias.double()
    t = temb.double()
    if mutation == "temb_row":
        t = t.clone()
        t[1] = t[0]
    y = y + t[:, None, None, :]
    if mutation == "drop_last_row":
        y[-1, -1, -1] = 0
    return y


def _exact_operands():
    s = SHAPE
    c = xo.conv_case(s["B"], s["N"], s["N"], s["C1"], s["C2"], s["Cout"], temb=True)
    return c, (c.x1, c.x2, c.w, c.bias, c.temb)


def test_restatement_is_the_reference():
    c, ops_ = _exact_operands()
    xo.assert_exact(restated_conv(*ops_), c.ref, "restated convolution")


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_exact_oracle_catches_each_planted_fault(mutation):
    c, ops_ = _exact_operands()
    with pytest.raises(AssertionError, match="differ from the float64 reference"):
        xo.assert_exact(restated_conv(*ops_, mutation=mutation).to(torch.bfloat16), c.ref, mutation)


@pytest.mark.parametrize("mutation", LOCALISED)
def test_loose_bf16_bound_misses_the_localised_faults(mutation):
    """The same faults on Gaussian operands of the same shapes pass close(..., torch.bfloat16) of tests/test_gpu_ops.py, a bf16 store
    of the result included: one of K = 13824 products moves an output by under 1 % of its sigma.  close() defaults to rel-RMS 1e-2;
    the convolution tests there call it with bf16_rms=6e-3 (max error 4.8e-2 of max|ref|), and that tighter bound is the one used
    here.  Measured: 4.0e-3 (tap channel), 3.8e-3 (halo corner), 5.2e-3 (seam) against 1.7e-3 for the bf16 store alone."""
    s = SHAPE
    g = torch.Generator().manual_seed(11)
    bf = lambda t: t.to(torch.bfloat16).float()
    K = 9 * (s["C1"] + s["C2"])
    x1, x2 = bf(torch.randn(s["B"], s["N"], s["N"], s["C1"], generator=g)), bf(torch.randn(s["B"], s["N"], s["N"], s["C2"], generator=g))
    w = bf(torch.randn(s["Cout"], 3, 3, s["C1"] + s["C2"], generator=g) / K ** 0.5)
    bias, temb = torch.randn(s["Cout"], generator=g), bf(torch.randn(s["B"], s["Cout"], generator=g))
    ref = restated_conv(x1, x2, w, bias, temb)
    got = restated_conv(x1, x2, w, bias, temb, mutation=mutation).to(torch.bfloat16)
    assert not torch.equal(got.double(), ref.to(torch.bfloat16).double()), "the fault changed nothing"
    close(got, ref, torch.bfloat16, mutation, bf16_rms=6e-3)
