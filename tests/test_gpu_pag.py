"""The two kernels of perturbed-attention guidance on MI355X, through the C ABI and the ops wrappers, against float64.

afldm_attn_identity_block (bf16): y = x + GN(x) W_vo^T + b_vo.  The float64 side uses the kernel's own rounded inputs - the bf16
x, the bf16 packed W_vo, mean and rstd finished in float64 from the same fp32 partial sums - so what is left is what the launch
itself rounds.  Per element, with A = sum_k |h_k| |W_nk| (h = GN(x) unrounded):
    tol = 2^-8 (A + |y|) + K 2^-24 A
the first term for the ONE bf16 rounding of the operand the launch forms (GN(x)) and for the output rounding, at 2^-8 rather than
2^-9 so that it also covers the fp32 finishing of mean and rstd; the second for the fp32 accumulation over K terms.  The same
ratio is printed for the two-launch composition (gn_apply + conv2d on the folded weight) as a yardstick; nothing is asserted on it.

afldm_pag_step / afldm_pag_step_flat: 2e-6 max|want|, the project's bound for the elementwise fp32 chain (test_sde_step_kernel),
plus, for phi > 0, 2 phi delta max|g| with delta = (log2(n) + 8) 2^-24 for the tree-reduced sums over a sample's n elements."""
import math

import pytest
import torch

import pag_oracle as po

pytestmark = pytest.mark.gpu

INF = math.inf
G, EPS = 32, 1e-5


# ------------------------------------------------------------------------------------------------ identity attention block
def _identity_inputs(B, T, C, dtype, seed):
    from afldm_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, T, C, generator=g) * 1.5 + 0.5).to("cuda", dtype)          # |mean| <= std per group
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).cuda()
    beta = (0.2 * torch.randn(C, generator=g)).cuda()
    w = ops.pack_weight((torch.randn(C, C, generator=g) / math.sqrt(C)).cuda(), dtype)
    bias = (0.1 * torch.randn(C, generator=g)).cuda()
    stats = ops.gn_stats(x, G)
    return x, stats, gamma, beta, w, bias


def _identity_reference(x, stats, gamma, beta, w, bias):
    """(y, A) in float64 from the kernel's own inputs."""
    B, T, C = x.shape
    s = stats.st1.double().sum(1).view(B, G, C // G, 2).sum(2)                    # [B, G, 2]
    n = (C // G) * T
    mean = s[..., 0] / n
    rstd = 1.0 / torch.sqrt((s[..., 1] / n - mean * mean).clamp_min(0) + EPS)
    xd = x.double()
    h = (xd.view(B, T, G, C // G) - mean[:, None, :, None]) * rstd[:, None, :, None]
    h = h.reshape(B, T, C) * gamma.double() + beta.double()
    wd = w.double().view(C, C)
    y = xd + h @ wd.T + bias.double()
    return y, h.abs() @ wd.abs().T


def _ratio(got, y, A, K):
    tol = 2.0 ** -8 * (A + y.abs()) + K * 2.0 ** -24 * A
    return float(((got.double() - y).abs() / tol).max())


@pytest.mark.parametrize("B,T,C", [(3, 4, 64), (2, 16, 128), (5, 64, 128), (1, 256, 384), (1, 1024, 192), (2, 4, 768)])
def test_identity_block_against_float64(B, T, C, monkeypatch):
    from afldm_amd import _lib, ops
    x, stats, gamma, beta, w, bias = _identity_inputs(B, T, C, torch.bfloat16, 100 + C + T)
    assert _lib.lib.afldm_attn_identity_block_ok(B, T, C, G, _lib.BF16) == 1
    out = torch.full_like(x, float("nan"))
    _lib.check(_lib.lib.afldm_attn_identity_block(x.data_ptr(), stats.st1.data_ptr(), stats.S1, gamma.data_ptr(), beta.data_ptr(), G,
                                                  EPS, w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, C, _lib.BF16,
                                                  _lib.stream_ptr()), "afldm_attn_identity_block")
    torch.cuda.synchronize()
    y, A = _identity_reference(x, stats, gamma, beta, w, bias)
    assert torch.isfinite(out).all()
    fused = _ratio(out, y, A, C)
    comp = ops.conv2d(ops.gn_apply(x, stats, gamma, beta, G, EPS, act=0), w, bias, residual=x)
    print(f"[identity block B={B} T={T} C={C}] error / bound: one launch {fused:.3f}, gn_apply + conv2d {_ratio(comp, y, A, C):.3f}")
    assert fused <= 1.0, fused
    # the wrapper: that launch where the policy sends the level to it (ops._IDENTITY_MIN_T), else the two launches
    via = ops.attn_identity_block(x, stats, gamma, beta, G, EPS, w, bias)
    assert torch.equal(via, out if ops.attn_identity_block_ok(x, G) else comp)
    monkeypatch.setattr(ops, "_IDENTITY_MIN_T", 4)
    assert ops.attn_identity_block_ok(x, G) and torch.equal(ops.attn_identity_block(x, stats, gamma, beta, G, EPS, w, bias), out)


def test_identity_block_fp32_runs_the_composition(monkeypatch):
    from afldm_amd import _lib, ops
    monkeypatch.setattr(ops, "_IDENTITY_MIN_T", 4)                     # (the policy aside: what the library has no kernel for)
    B, T, C = 2, 16, 128
    x, stats, gamma, beta, w, bias = _identity_inputs(B, T, C, torch.float32, 7)
    assert _lib.lib.afldm_attn_identity_block_ok(B, T, C, G, _lib.F32) == 0 and not ops.attn_identity_block_ok(x, G)
    got = ops.attn_identity_block(x, stats, gamma, beta, G, EPS, w, bias)
    comp = ops.conv2d(ops.gn_apply(x, stats, gamma, beta, G, EPS, act=0), w, bias, residual=x)
    assert torch.equal(got, comp)
    y, A = _identity_reference(x, stats, gamma, beta, w, bias)
    # fp32 throughout: one rounding of GN(x), K accumulated terms, the output rounding
    tol = 2.0 ** -23 * (A + y.abs()) + C * 2.0 ** -24 * A
    assert float(((got.double() - y).abs() / tol).max()) <= 1.0
    # a shape without a kernel takes the same route in bf16
    xb, sb, gb, bb, wb, biasb = _identity_inputs(2, 32, 128, torch.bfloat16, 8)
    assert not ops.attn_identity_block_ok(xb, G)
    assert torch.equal(ops.attn_identity_block(xb, sb, gb, bb, G, EPS, wb, biasb),
                       ops.conv2d(ops.gn_apply(xb, sb, gb, bb, G, EPS, act=0), wb, biasb, residual=xb))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_identity_block_out_slice_leaves_the_other_half(dtype, monkeypatch):
    from afldm_amd import ops
    monkeypatch.setattr(ops, "_IDENTITY_MIN_T", 4)                     # bf16: the one launch; fp32: the two launches
    B, T, C = 3, 16, 64
    x, stats, gamma, beta, w, bias = _identity_inputs(B, T, C, dtype, 9)
    want = ops.attn_identity_block(x, stats, gamma, beta, G, EPS, w, bias)
    buf = torch.full((2 * B, T, C), 7.0, dtype=dtype, device="cuda")
    got = ops.attn_identity_block(x, stats, gamma, beta, G, EPS, w, bias, out=buf[B:])
    assert got.data_ptr() == buf[B:].data_ptr()
    assert torch.equal(buf[B:], want) and bool((buf[:B] == 7.0).all())


# ------------------------------------------------------------------------------------------------ guided update
BASE = (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.0, 0.7, 0.5)
ROWS = [
    BASE + (0.0, 0.0, 0.0, 0.0, 0.0),                              # s = 0, phi = 0: the stochastic row applied to e
    BASE + (0.0, 3.0, 0.0, 0.0, 0.0),                              # s = 3
    BASE + (0.0, 3.0, 0.7, 0.0, 0.0),                              # s = 3 with the rescale
    (1.0, -0.9, -1.0, 1.0, 0.4, 0.55, 0.0, 0.0, 3.0, 0.7, 0.0, 0.0),      # a clamping row
    BASE + (0.3, 3.0, 0.7, 0.0, 0.0),                              # c != 0: the noise row is read
]


def _f32(row):
    return [float(v) for v in torch.tensor(row, dtype=torch.float32)]


def _bound(want, x, e, ep, row, label):
    s, phi = row[8], row[9]
    n = x[0].numel()
    first = 2e-6 * float(want.abs().max())
    gmax = float(po.pag_step(x, e, ep, None, (0.0, 0.0, -INF, INF, 0.0, 0.0, 1.0, 0.0, s, phi)).abs().max())
    second = 2.0 * phi * (math.log2(n) + 8) * 2.0 ** -24 * gmax if phi > 0 else 0.0
    return first, second


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 4, 16, 16), (2, 3, 5, 5), (2, 4, 32, 32), (1, 4, 64, 64)])
def test_pag_step_kernels(dtype, shape):
    from afldm_amd import ops
    B = shape[0]
    g = torch.Generator().manual_seed(23)
    x = torch.randn(*shape, generator=g)
    e = torch.randn(*shape, generator=g).to(dtype).float()                        # what the kernels read
    ep = (e + 0.3 * torch.randn(*shape, generator=g)).to(dtype).float()
    eps2 = torch.cat([e, ep]).permute(0, 2, 3, 1).contiguous().to("cuda", dtype)
    big = torch.randn(len(ROWS), 2 * B, *shape[1:], generator=g)                   # the noise rows as a batch slice of a larger buffer
    noise = big.cuda()[:, B:]
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    for k, row in enumerate(ROWS):
        r = _f32(row)
        want = po.pag_step(x, e, ep, big[k, B:], r)
        first, second = _bound(want, x.double(), e.double(), ep.double(), r, k)
        idx = torch.full((1,), k, dtype=torch.int32, device="cuda")
        xg = x.cuda()
        out = ops.pag_step(xg, eps2, noise, coef, idx, advance=False, out=xg)      # x_out aliases x
        assert out.data_ptr() == xg.data_ptr() and int(idx.item()) == k
        err = float((out.cpu().double() - want).abs().max())
        print(f"[pag_step {tuple(shape)} {dtype} row {k}] error {err:.3e}; bound {first:.3e} + {second:.3e}")
        assert err <= first + second, (k, err, first, second)
        if dtype == torch.float32:                                                 # the eager loop's form: same-layout fp32 tensors
            flat = ops.pag_step_flat(x.cuda(), e.cuda(), ep.cuda(), noise[k].contiguous() if r[7] else None, r)
            errf = float((flat.cpu().double() - want).abs().max())
            print(f"[pag_step_flat {tuple(shape)} row {k}] error {errf:.3e}")
            assert errf <= first + second, (k, errf, first, second)
        if r[7] == 0.0:                                                            # c = 0: no noise pointer is needed
            assert torch.equal(ops.pag_step(x.cuda(), eps2, None, coef, idx), out)
    # advance: the kernel reads row 0, then the counter moves on; a second launch reads row 1
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    ops.pag_step(xg, eps2, noise, coef, idx, advance=True, out=xg)
    ops.pag_step(xg, eps2, noise, coef, idx, advance=True, out=xg)
    assert int(idx.item()) == 2
    want = po.pag_step(po.pag_step(x, e, ep, None, _f32(ROWS[0])), e, ep, None, _f32(ROWS[1]))
    assert float((xg.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_pag_step_ratio_edges():
    from afldm_amd import ops
    shape = (3, 4, 16, 16)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(*shape, generator=g).cuda()
    e = torch.randn(*shape, generator=g)
    same = torch.cat([e, e]).permute(0, 2, 3, 1).contiguous().cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = torch.tensor(BASE + (0.0, 3.0, 1.0, 0.0, 0.0), dtype=torch.float32).cuda()
    off = torch.tensor(BASE + (0.0, 3.0, 0.0, 0.0, 0.0), dtype=torch.float32).cuda()
    # e_p == e: g = e exactly, sigma(g) = sigma(e) in the same bits, the ratio is exactly 1
    assert torch.equal(ops.pag_step(x, same, None, one, idx), ops.pag_step(x, same, None, off, idx))
    assert torch.equal(ops.pag_step_flat(x, e.cuda(), e.cuda(), None, one.tolist()), ops.pag_step_flat(x, e.cuda(), e.cuda(), None, off.tolist()))
    # one sample with g == 0: the ratio is defined as 1 there, and nothing is NaN
    e0 = e.clone()
    e0[1] = 0.0
    zero = torch.cat([e0, e0]).permute(0, 2, 3, 1).contiguous().cuda()
    r = torch.tensor(BASE + (0.0, 3.0, 0.7, 0.0, 0.0), dtype=torch.float32)
    out = ops.pag_step(x, zero, None, r.cuda(), idx).cpu()
    want = po.pag_step(x.cpu(), e0, e0, None, r.tolist())
    assert torch.isfinite(out).all()
    assert float((out.double() - want).abs().max()) <= 2e-6 * float(want.abs().max()) + 2 * 0.7 * 18 * 2.0 ** -24 * float(e0.abs().max())


def test_pag_step_refuses_a_sample_above_the_element_limit():
    from afldm_amd import _lib, ops
    shape = (1, 4, 64, 68)                                                         # 17408 elements; the limit is 16384
    x = torch.zeros(*shape, device="cuda")
    eps2 = torch.zeros(2, 64, 68, 4, device="cuda")
    coef = torch.tensor(ROWS[0], dtype=torch.float32).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.AfldmError):
        ops.pag_step(x, eps2, None, coef, idx)
    with pytest.raises(_lib.AfldmError):
        ops.pag_step_flat(x, x.clone(), x.clone(), None, ROWS[0])
    torch.cuda.synchronize()
