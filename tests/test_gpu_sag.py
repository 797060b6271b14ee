"""The two kernels of self-attention guidance on MI355X, through the C ABI and the ops wrappers, against float64.

afldm_attn_key_mass: mass[b, j] = (1 / heads) sum_h sum_i softmax_j(scale q_bhi . k_bhj).  The float64 side is computed from the
kernel's own (rounded) q and k, so what is left is what the launches round.  Per key, with M_j the float64 mass and
a_max = max_ij scale sum_k |q_ik| |k_jk|:
    tol_j = 2^-24 M_j ((d + 8) a_max + 2 T + heads + 16)
(d + 8) a_max: fp32 accumulation of a score over d terms, the scaling, the subtraction of the row maximum and the exponential's
argument and result, all relative to the exponent's magnitude; 2 T: the sequential worst case of a row sum and of a column sum;
heads + 16: the sum over the heads, the reciprocal, the product with it and the final division.

afldm_sag_degrade / _flat: with fp32 output 4e-6 max(max|x|, max|x0| / p) - the project's 2e-6 for an elementwise fp32 chain
(test_sde_step_kernel) plus 18 taps of 2^-24, rounded up; with bf16 output 2^-8 |want| is added for the output rounding."""
import pytest
import torch

import sag_oracle as so

pytestmark = pytest.mark.gpu

ESHAPE = -1


# ------------------------------------------------------------------------------------------------ key mass
def _qk(B, heads, T, d, dtype, halves, gain, seed):
    """(q, k) on the device as the kernel reads them: the two column halves of one [B, T, 2 C] buffer, or contiguous tensors."""
    C = heads * d
    g = torch.Generator().manual_seed(seed)
    qk = (torch.randn(B, T, 2 * C, generator=g) * gain).to("cuda", dtype)
    if halves:
        return qk[:, :, :C], qk[:, :, C:]
    return qk[:, :, :C].contiguous(), qk[:, :, C:].contiguous()


def _key_mass_reference(q, k, heads):
    """(mass float64 [B, T], a_max) from the rounded operands."""
    B, T, C = q.shape
    d = C // heads
    qd, kd = q.detach().cpu().double(), k.detach().cpu().double()
    mass = so.key_mass(qd, kd, heads)
    qa = qd.abs().view(B, T, heads, d).transpose(1, 2)
    ka = kd.abs().view(B, T, heads, d).transpose(1, 2)
    a_max = float((qa @ ka.transpose(-1, -2)).max()) * d ** -0.5
    return mass, a_max


def _key_mass_tol(mass, a_max, heads, T, d):
    return 2.0 ** -24 * mass * ((d + 8) * a_max + 2 * T + heads + 16)


CASES = [(2, 32, 4, 24, 1.0), (3, 8, 16, 16, 1.0), (2, 8, 64, 16, 3.7), (1, 16, 64, 24, 1.0), (2, 4, 256, 16, 1.0),
         (1, 16, 256, 24, 1.0), (1, 8, 1024, 24, 1.0)]


@pytest.mark.parametrize("halves", [True, False], ids=["halves", "contiguous"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,heads,T,d,gain", CASES)
def test_key_mass_against_float64(B, heads, T, d, gain, dtype, halves):
    from afldm_amd import _lib, ops
    q, k = _qk(B, heads, T, d, dtype, halves, gain, 1000 + T + d)
    assert q.is_contiguous() != halves and _lib.lib.afldm_attn_key_mass_ok(B, heads, T, d, _lib.DTYPE_CODE[dtype]) == 1
    assert ops.attn_key_mass_ok(q, heads)
    want, a_max = _key_mass_reference(q, k, heads)
    if gain > 1.0:      # the case whose scaled scores reach about +-60: a softmax without its maximum subtracted overflows here
        qh = q.double().view(B, T, heads, d).transpose(1, 2).cpu()
        kh = k.double().view(B, T, heads, d).transpose(1, 2).cpu()
        s = qh @ kh.transpose(-1, -2) * d ** -0.5
        assert float(s.max()) > 45.0 and float(s.min()) < -45.0, (float(s.min()), float(s.max()))
    out = torch.full((B, T), float("nan"), device="cuda")
    got = ops.attn_key_mass(q, k, heads, out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().double()
    assert torch.isfinite(got).all()
    tol = _key_mass_tol(want, a_max, heads, T, d)
    ratio = float(((got - want).abs() / tol).max())
    total = float((got.sum(1) - T).abs().max())
    print(f"[key mass B={B} heads={heads} T={T} d={d} {dtype} {'halves' if halves else 'contiguous'}] a_max {a_max:.1f}; "
          f"error / bound {ratio:.3f}; |sum_j mass - T| {total:.2e} (bound {float(tol.sum(1).min()):.2e})")
    assert ratio <= 1.0, ratio
    assert bool(((got.sum(1) - T).abs() <= tol.sum(1)).all())             # a row of P sums to 1: the masses sum to T
    # a sample's bits depend neither on B nor on its place in the batch
    if B > 1:
        assert torch.equal(ops.attn_key_mass(q[:1], k[:1], heads)[0], out[0])
        assert torch.equal(ops.attn_key_mass(q[B - 1:], k[B - 1:], heads)[0], out[B - 1])
    assert torch.equal(ops.attn_key_mass(q, k, heads, scale=d ** -0.5), out)      # a repeat, bit for bit


def test_key_mass_of_a_uniform_map_is_one():
    from afldm_amd import ops
    q = torch.zeros(2, 64, 128, device="cuda")
    k = torch.randn(2, 64, 128, device="cuda")
    mass = ops.attn_key_mass(q, k, 8)
    assert float((mass - 1.0).abs().max()) <= 2.0 ** -24 * (2 * 64 + 8 + 16)


def test_key_mass_refuses_shapes_without_a_kernel():
    from afldm_amd import _lib, ops
    lib = _lib.lib
    for B, heads, T, d in ((1, 4, 64, 40), (1, 4, 12, 16)):
        C = heads * d
        assert lib.afldm_attn_key_mass_ok(B, heads, T, d, _lib.BF16) == 0 and lib.afldm_attn_key_mass_ok(B, heads, T, d, _lib.F32) == 0
        q = torch.zeros(B, T, C, device="cuda")
        mass = torch.full((B, T), 7.0, device="cuda")
        ws = torch.zeros(B * heads * T * 2, device="cuda")
        rc = lib.afldm_attn_key_mass(q.data_ptr(), C, q.data_ptr(), C, mass.data_ptr(), ws.data_ptr(), B, heads, T, d, d ** -0.5,
                                     _lib.F32, _lib.stream_ptr())
        assert rc == ESHAPE
        assert not ops.attn_key_mass_ok(q, heads)
        with pytest.raises(_lib.AfldmError):
            ops.attn_key_mass(q, q, heads)
        torch.cuda.synchronize()
        assert bool((mass == 7.0).all())                                   # refused before any launch


# ------------------------------------------------------------------------------------------------ degradation
P, Q = 1.0 / 0.6, -0.8 / 0.6
DEGRADE = [(2, 4, 16, 4, 9), (3, 4, 32, 8, 15), (1, 4, 8, 2, 9), (1, 4, 64, 64, 9), (2, 4, 16, 16, 1)]


def _masses(B, hm, g):
    """fp32 masses at least 1e-3 away from 1, plus three entries that must not be masked: exactly 1, a NaN, 1 - 2^-24."""
    u = torch.rand(B, hm * hm, generator=g)
    sign = torch.where(torch.rand(B, hm * hm, generator=g) > 0.5, 1.0, -1.0)
    mass = (1.0 + sign * (1e-3 + 0.1 * u)).float()
    mass[0, 0], mass[0, 1], mass[0, 2] = 1.0, float("nan"), 1.0 - 2.0 ** -24
    assert float(mass[0, 2]) < 1.0
    return mass


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("boundary", ["reflect", "circular"])
@pytest.mark.parametrize("B,C,H,hm,ntaps", DEGRADE)
def test_degrade_against_float64(B, C, H, hm, ntaps, boundary, dtype):
    from afldm_amd import ops
    g = torch.Generator().manual_seed(31 + H + hm)
    x = torch.randn(B, C, H, H, generator=g)
    e = torch.randn(B, C, H, H, generator=g).to(dtype).float()            # what the kernel reads
    mass = _masses(B, hm, g)
    taps = ops.gaussian_taps(ntaps, 1.0)
    rows = torch.tensor([[9.0, 9.0] + [0.0] * 10, [P, Q] + [0.0] * 10, [7.0, 7.0] + [0.0] * 10], dtype=torch.float32)
    p, q = float(rows[1, 0]), float(rows[1, 1])                           # the fp32 values the kernel reads
    mask = mass > 1.0
    assert not mask[0, :3].any() and mask.any()
    window = torch.tensor(taps, dtype=torch.float64)
    want = so.degrade(x, e, mask, p, q, window, boundary)                 # diffusers' form, float64
    x0 = p * x.double() + q * e.double()
    bound = 4e-6 * max(float(x.abs().max()), float(x0.abs().max()) / p)
    idx = torch.full((1,), 1, dtype=torch.int32, device="cuda")
    e_nhwc = e.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)
    got = ops.sag_degrade(x.cuda(), e_nhwc, mass.cuda(), taps, boundary, rows.reshape(-1).cuda(), idx)
    assert got.dtype == dtype and tuple(got.shape) == (B, H, H, C) and int(idx.item()) == 1
    got_nchw = got.permute(0, 3, 1, 2).cpu()
    err = (got_nchw.double() - want).abs()
    tol = bound + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0.0)
    print(f"[sag_degrade B={B} C={C} H={H} hm={hm} taps={ntaps} {boundary} {dtype}] max error {float(err.max()):.3e}; fp32 bound "
          f"{bound:.3e}; {100 * float(mask.float().mean()):.0f} % of the tokens masked")
    assert bool((err <= tol).all()), float((err - tol).max())
    # unmasked elements are the to_nhwc conversion of x, bit for bit
    M = so.upsampled_mask(mask, H, H).expand(B, C, H, H) > 0
    plain = ops.to_nhwc(x.cuda(), dtype).permute(0, 3, 1, 2).cpu()
    assert torch.equal(got_nchw[~M], plain[~M])
    if ntaps == 1:
        assert torch.equal(got_nchw, plain)                                # the identity blur: x_d is x
    else:
        assert not torch.equal(got_nchw[M], plain[M])
    if dtype == torch.float32:
        flat = ops.sag_degrade_flat(x.cuda(), e.cuda(), mass.cuda(), taps, boundary, p, q)
        assert torch.equal(flat.cpu(), got_nchw)                           # one device function, one arithmetic order
        assert bool(((flat.cpu().double() - want).abs() <= bound).all())


def test_degrade_refuses_before_any_launch():
    from afldm_amd import _lib, ops
    taps = ops.gaussian_taps()
    coef = torch.tensor([P, Q] + [0.0] * 10, dtype=torch.float32).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(B, C, H, W, T, taps=taps):
        x = torch.zeros(B, C, H, W, device="cuda")
        e = torch.zeros(B, H, W, C, device="cuda")
        mass = torch.full((B, T), 2.0, device="cuda")
        with pytest.raises(_lib.AfldmError):
            ops.sag_degrade(x, e, mass, taps, "reflect", coef, idx)
        with pytest.raises(_lib.AfldmError):
            ops.sag_degrade_flat(x, x.clone(), mass, taps, "reflect", P, Q)

    call(1, 4, 16, 24, 16)                 # H != W
    call(1, 4, 4, 4, 4)                    # H < 8
    call(1, 2, 72, 72, 36)                 # H > 64
    call(1, 8, 64, 64, 64)                 # C H W > 16384
    call(1, 4, 16, 16, 9)                  # hm = 3 does not divide 16
    call(1, 4, 16, 16, 16, taps=taps[:8])              # an even tap count
    call(1, 4, 16, 16, 16, taps=(1.0 / 17,) * 17)      # more than 15 taps
    with pytest.raises(ValueError):
        ops.sag_degrade_flat(torch.zeros(1, 4, 16, 16, device="cuda"), torch.zeros(1, 4, 16, 16, device="cuda"),
                             torch.zeros(1, 16, device="cuda"), taps, "zeros", P, Q)
    # the C ABI says why: AFLDM_ESHAPE
    x = torch.zeros(1, 4, 16, 24, device="cuda")
    w = (_lib.ctypes.c_float * 9)(*taps)
    rc = _lib.lib.afldm_sag_degrade_flat(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), P, Q, w, 9, 0, 1, 4, 16, 24, 4,
                                         _lib.stream_ptr())
    assert rc == ESHAPE
    torch.cuda.synchronize()
