"""The GroupNorm partial-sum oracle checked against itself and against PyTorch on the CPU (no GPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_oracle as go

RATIOS = [0.5, 8, 32, 128]
DTYPES = [torch.float32, torch.bfloat16]


def _case(ratio, dtype, B=3, C=32, G=4, HW=64, seed=5, const=0.25):
    gen = torch.Generator().manual_seed(seed)
    x = go.hard_planes(B, C, G, HW, ratio, seed, dtype, const=const)
    gamma = 1 + 0.2 * torch.randn(C, generator=gen)
    beta = 0.5 * torch.randn(C, generator=gen)
    return x, gamma, beta


@pytest.mark.parametrize("ratio", RATIOS)
def test_finish_on_exact_partials_is_group_norm(ratio):
    """With float64 partial sums (no fp32 rounding of the format) finish + apply IS F.group_norm in float64."""
    B, C, G, HW, eps = 3, 32, 4, 64, 1e-5
    x, gamma, beta = _case(ratio, torch.float32)
    cuts = go.ragged_cuts(HW, 5, 1)
    xd = x.double()
    st = torch.stack([torch.stack([xd[:, a:b].sum(1), (xd[:, a:b] ** 2).sum(1)], -1) for a, b in zip(cuts, cuts[1:])], 1)
    s = st.sum(1).view(B, G, C // G, 2).sum(2)
    n = HW * C // G
    mean = s[..., 0] / n
    rstd = 1 / torch.sqrt((s[..., 1] / n - mean * mean).clamp_min(0) + eps)
    got = go.apply(x, mean, rstd, gamma, beta, G)
    ref = F.group_norm(xd.transpose(1, 2), G, gamma.double(), beta.double(), eps).transpose(1, 2)
    # s2/n - m^2 in float64 cancels (ratio / std)^2 ~ 2^14..2^16 at ratio 128: 2^-53 * 2^16 relative in var, 1e-11 with margin
    assert ((got - ref).abs() / (1 + ref.abs())).max() <= 1e-11 * max(1.0, ratio) ** 2
    assert ((go.true_groupnorm(x, gamma, beta, G, eps) - ref).abs() / (1 + ref.abs())).max() <= 1e-11 * max(1.0, ratio) ** 2
    # finish() on the fp32 format takes the same route: identical when the partials are exact (integers)
    xi = go.int_planes(B, C, HW, 3, torch.bfloat16)
    m1, r1 = go.finish(go.partials(xi, cuts), None, G, n, eps)
    refi = F.group_norm(xi.double().transpose(1, 2), G, gamma.double(), beta.double(), eps).transpose(1, 2)
    assert (go.apply(xi, m1, r1, gamma, beta, G) - refi).abs().max() <= 1e-12 * (1 + refi.abs().max())


def _kernel_formula_fp32(x, st1, st2, gamma, beta, G, n, eps, dtype):
    """k_gn_apply's arithmetic in numpy fp32: sums and s2/n - m^2 in fp64, var cast to fp32, rsqrtf(var + eps), k = rstd gamma,
    sh = beta - mean k, y = x k + sh (two roundings), stored in `dtype`."""
    s = go.group_sums(st1, st2, G).numpy()
    m = s[..., 0] / n
    var32 = np.maximum((s[..., 1] / n - m * m).astype(np.float32), np.float32(0))
    rstd = (np.float32(1) / np.sqrt((var32 + np.float32(eps)).astype(np.float64))).astype(np.float32)
    mean = m.astype(np.float32)
    cpg = x.shape[-1] // G
    k = (np.repeat(rstd, cpg, 1) * gamma.numpy()).astype(np.float32)
    sh = (beta.numpy() - (np.repeat(mean, cpg, 1) * k).astype(np.float32)).astype(np.float32)
    y = ((x.numpy() * k[:, None, :]).astype(np.float32) + sh[:, None, :]).astype(np.float32)
    return torch.from_numpy(y).to(dtype).double()


@pytest.mark.parametrize("const", [0.25, "loud"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ratio", RATIOS)
def test_fp32_kernel_formula_stays_inside_apply_bound(ratio, dtype, const):
    B, C, G, HW, eps = 3, 32, 4, 64, 1e-5
    x, gamma, beta = _case(ratio, dtype, const=const)
    C1 = 12                                                   # a concat whose seam falls inside group 1
    st1 = go.partials(x[..., :C1].contiguous(), go.ragged_cuts(HW, 9, 2))
    st2 = go.partials(x[..., C1:].contiguous(), go.ragged_cuts(HW, 4, 3))
    n = HW * C // G
    worst = 0.0
    for a, b in ((st1, st2), (go.starved(st1, G, C, 0), go.starved(st2, G, C, C1))):
        mean, rstd = go.finish(a, b, G, n, eps)
        ref = go.apply(x, mean, rstd, gamma, beta, G)
        k, sh = go.scale_shift(mean, rstd, gamma, beta, G)
        got = _kernel_formula_fp32(x, a, b, gamma, beta, G, n, eps, dtype)
        frac = ((got - ref).abs() / go.apply_bound(x, k, sh, ref, dtype)).max().item()
        worst = max(worst, frac)
    print(f"ratio {ratio} {dtype}: worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_int_planes_meet_their_cap():
    for dtype in DTYPES:
        x = go.int_planes(3, 8, 4096, 0, dtype)
        assert x.abs().max() <= go.MAX_INT and torch.equal(x, x.round())
        st = go.partials(x, go.ragged_cuts(4096, 3, 0)).double()
        assert st.abs().max() < go.MAX_SUM and torch.equal(st, st.round())
        assert torch.equal(st.sum(1)[..., 1], (x.double() ** 2).sum(1))
    with pytest.raises(AssertionError):
        go.int_planes(1, 4, 1 << 18, 0, torch.float32)


@pytest.mark.parametrize("ratio", RATIOS)
def test_starved_partials_have_a_negative_raw_variance(ratio):
    B, C, G, HW = 3, 32, 4, 65
    for dtype, const in [(d, c) for d in DTYPES for c in (0.25, "loud")]:
        x = go.hard_planes(B, C, G, HW, ratio, 11, dtype, const=const)
        b, g = go.const_key(B, G)
        n = HW * C // G
        for S in (1, 9):
            st = go.partials(x, go.ragged_cuts(HW, S, S))
            s = go.group_sums(st, None, G)
            raw = s[..., 1] / n - (s[..., 0] / n) ** 2
            assert raw[b, g] == 0.0                            # exactly constant, exactly summed
            hungry = go.starved(st, G)
            s = go.group_sums(hungry, None, G)
            raw2 = s[..., 1] / n - (s[..., 0] / n) ** 2
            assert raw2[b, g] < 0.0
            mask = torch.ones(B, G, dtype=torch.bool)
            mask[b, g] = False
            assert torch.equal(raw2[mask], raw[mask])          # nothing else moved
            assert go.finish(hungry, None, G, n, 1e-6)[1][b, g] == 1e-6 ** -0.5   # the clamp of the reference


def test_format_rstd_error_table():
    """What the fp32 partial-sum FORMAT loses in rstd against float64 statistics of the same data (see gn_oracle's docstring,
    where the printed figures are recorded).  Asserted only where the end-to-end GPU check works: ratio <= 8."""
    B, C, G, HW, eps = 3, 32, 4, 64, 1e-5
    n = HW * C // G
    table = {}
    for ratio in RATIOS:
        x = go.hard_planes(B, C, G, HW, ratio, 5, torch.float32)
        _, rstd = go.finish(go.partials(x, go.even_cuts(HW, 4)), None, G, n, eps)
        xg = x.double().view(B, HW, G, C // G)
        var = ((xg - xg.mean((1, 3), keepdim=True)) ** 2).mean((1, 3))
        true = 1 / torch.sqrt(var + eps)
        mask = torch.ones(B, G, dtype=torch.bool)
        mask[go.const_key(B, G)] = False                       # rstd = eps^-1/2 on both sides there
        table[ratio] = ((rstd - true).abs() / true)[mask].max().item()
    print("format rstd error:", {k: f"{v:.2e}" for k, v in table.items()})
    assert table[0.5] <= 2e-6 and table[8] <= 2e-6
    for ratio in RATIOS:                                       # the docstring's record is this table (to one digit)
        assert 0.3 * go.FORMAT_RSTD_ERR[ratio] <= max(table[ratio], 1e-9) <= 3 * go.FORMAT_RSTD_ERR[ratio]


# ------------------------------------------------------------------------------------------------ planted faults
# What a consumer with one of the slips named in test_gpu_groupnorm_stats' docstring would hand back, formed on the CPU from
# the GPU file's own cases (same data, same cuts, same split matrix): each must leave the bound that file asserts.
def _unmasked(st, smax):
    """Reading splits 0 .. smax - 1 of a tensor that has S < smax of them: the addresses run on into the next sample's partials
    (zeros behind the last sample's, the kindest outcome)."""
    B, S, C, _ = st.shape
    flat = torch.cat([st.reshape(-1), torch.zeros(smax * C * 2)])
    idx = (torch.arange(B)[:, None, None, None] * S + torch.arange(smax)[None, :, None, None]) * C * 2 \
        + torch.arange(C)[None, None, :, None] * 2 + torch.arange(2)[None, None, None, :]
    return flat[idx]


def _fault_ratio(case, st1, st2):
    """max |faulty - ref| / apply_bound with the faulty consumer's statistics."""
    n = case.HW * case.C // case.G
    mean, rstd = go.finish(st1, st2, case.G, n, case.eps)
    got = go.apply(case.x, mean, rstd, case.gamma, case.beta, case.G).float().to(case.dtype).double()
    return ((got - case.ref).abs() / go.apply_bound(case.x, case.k, case.sh, case.ref, case.dtype)).max().item()


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_consumer_faults_leave_the_bound(dtype):
    import test_gpu_groupnorm_stats as gs
    small = [s for s in gs.APPLY_SHAPES if s[4] * s[3] * (s[0] + s[1]) <= 1 << 15 and dtype in s[5]]
    assert len(small) >= 6
    tail_seen = {S: 0 for S in gs.SINGLE_S}
    for C1, C2, G, HW, B, _ in small:
        for ratio, starve, const in gs.VARIANTS:
            for S1, S2 in gs._split_matrix(C2):
                c = gs.Case(B, C1, C2, G, HW, dtype, ratio, starve, const, S1, S2, seed=ratio)
                assert _fault_ratio(c, c.st1, c.st2) <= 1.0                                  # the faultless consumer
                # (a) the statistics of sample b + 1 for sample b
                assert _fault_ratio(c, c.st1.roll(-1, 0), None if c.st2 is None else c.st2.roll(-1, 0)) > 1.0
                # (b) `sp < S` not applied: the tensor with fewer splits is read up to max(S1, S2)
                if C2 and S1 != S2:
                    smax = max(S1, S2)
                    a, b = (_unmasked(c.st1, smax), c.st2) if S1 < S2 else (c.st1, _unmasked(c.st2, smax))
                    assert _fault_ratio(c, a, b) > 1.0, (C1, C2, S1, S2)
                # (c) the S % 8 tail of gn_channel_sums dropped
                if not C2 and S1 % 8:
                    cut = c.st1[:, :S1 - S1 % 8] if S1 > 8 else torch.zeros_like(c.st1)
                    tail_seen[S1] += _fault_ratio(c, cut, None) > 1.0
    # ragged_cuts keeps a pixel in the last split, so a lost tail is seen at every tail length (1, 3, 8 + 1, 16 + 1) in every case
    nsingle = 3 * sum(1 for s in small if not s[1])
    assert all(tail_seen[S] == nsingle for S in (1, 3, 9, 17)), tail_seen


def test_planted_split_boundary_is_seen_by_the_exact_producer_cases():
    """k_gn_partial with p0 = (HW / S) * sp or ceil(HW / S) * sp instead of HW * sp / S: wherever such a rule moves a boundary,
    the integer planes give different partials (no boundary moves unseen), and at every ragged HW of test_gn_stats_exact at least
    one of the two rules does move one."""
    import test_gpu_groupnorm_stats as gs
    for HW in gs.HWS:
        S = 32 if HW >= 1024 else 16 if HW >= 256 else 4 if HW >= 64 else 1
        x = go.int_planes(3, 8, HW, HW, torch.bfloat16)
        right = go.even_cuts(HW, S)
        moved = 0
        for step in (HW // S, -(-HW // S)):
            wrong = [min(step * s, HW) for s in range(S)] + [HW]
            same = torch.equal(go.partials(x, wrong), go.partials(x, right))
            assert same == (wrong == right), (HW, step)
            moved += wrong != right
        assert (moved > 0) == (HW % S != 0), HW
