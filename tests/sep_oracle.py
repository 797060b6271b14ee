"""CPU oracle of the large-plane kernels of csrc/sep.hip (afldm_sep_pass, afldm_gn_table, afldm_softmax_rows) and of
afldm_gn_fold, the seeded input recipes of their tests, a per-group error measure, and a CPU model of the bf16 roundings.

Layout of a pass: x [outer, K, inner] - `inner` memory-adjacent lines of K samples each (a line is a strided vector along k);
y [outer, R or R2, inner].  The kernel's W form (lines = channels of one pixel row) and H form (lines = (w, c) pairs of one
sample) are both this layout, with few / many lines per outer.  16 CT adjacent lines form one group, the unit of work of a wave.

Every recipe returns fp32 tensors that were ROUNDED THROUGH the test dtype, so the oracle and the kernel see identical numbers;
the oracle itself is float64 and written out plainly as einsum.

Tolerances (TOL) are the project's own for these kernels (test_gpu_vae.py), applied PER GROUP of 16 lines instead of over the
whole tensor: rel-RMS fp32 2e-5; bf16 8e-3 for a plain pass, 1.2e-2 for a chained pass, 1.5e-2 for the composed activation."""
import torch

TOL = {"fp32": 2e-5, "plain": 8e-3, "chained": 1.2e-2, "composed": 1.5e-2}

# the dispatch table of sep_dispatch (csrc/sep.hip): (K, R, R2)
PLAIN = [(16, 32, 0), (32, 64, 0), (64, 128, 0), (32, 16, 0), (64, 32, 0), (128, 64, 0)]
CHAINED = [(16, 32, 16), (32, 64, 32), (64, 128, 64)]
BF16_ONLY = [(128, 256, 0), (256, 128, 0), (128, 256, 128)]
CT = {(128, 256): 4, (256, 128): 2, (64, 128): 4, (128, 64): 2, (32, 64): 4, (64, 32): 4}     # bf16 plain passes, 16 CT lines per wave
SWEEP_GROUPS = 4099                  # 2 * 2048 + 3 = 4 * 1024 + 3: past two sweeps of the largest grid, three live waves at the end


def configs(dtype):
    return PLAIN + CHAINED + (BF16_ONLY if dtype == torch.bfloat16 else [])


def tol(dtype, R2=0, composed=False):
    if dtype == torch.float32:
        return TOL["fp32"]
    return TOL["composed"] if composed else TOL["chained"] if R2 else TOL["plain"]


def rnd(x, dtype):
    return x.to(dtype).to(torch.float32)


def matrices(K, R, R2=0):
    """The project's own host fp32 filter matrices: M [R, K] (x2 upsampler U for R = 2K, low-pass decimator D for R = K/2)
    and, for a chained pass, M2 = D [R/2, R]."""
    from afldm_amd import _lib
    assert R == 2 * K or 2 * R == K, (K, R)
    M = _lib.filter_matrix(0, K, 2) if R == 2 * K else _lib.filter_matrix(1, K)
    M2 = None
    if R2:
        assert 2 * R2 == R
        M2 = _lib.filter_matrix(1, R)
    assert tuple(M.shape) == (R, K) and (M2 is None or tuple(M2.shape) == (R2, R))
    return M, M2


# ------------------------------------------------------------------------------------------------ the oracle
def silu64(z):
    return z / (1.0 + torch.exp(-z))


def normalised(x, table=None, C=0, outer_per_sample=1):
    """xn = x * scale[b, line % C] + shift[b, line % C], b = outer // outer_per_sample (float64)"""
    x = x.double()
    if table is None:
        return x
    outer, K, inner = x.shape
    b = torch.arange(outer) // outer_per_sample
    c = torch.arange(inner) % C
    t = table.double()[b][:, c]                                     # [outer, inner, 2]
    return x * t[:, None, :, 0] + t[:, None, :, 1]


def sep_reference(x, M, M2=None, act=0, table=None, C=0, outer_per_sample=1):
    xn = normalised(x, table, C, outer_per_sample)
    z = torch.einsum("rk,oki->ori", M.double(), xn)
    if M2 is not None:
        return torch.einsum("sr,ori->osi", M2.double(), silu64(z))
    return silu64(z) if act else z


def gn_table_reference(st, gamma, beta, G, HW, eps):
    """[B, C, 2] float64 (scale, shift) = (rstd gamma, beta - mean rstd gamma) from partial sums st [B, S, C, 2]"""
    s = st.double().sum(1)                                          # [B, C, 2]
    B, C, _ = s.shape
    cpg = C // G
    grp = s.view(B, G, cpg, 2).sum(2)
    n = float(HW) * cpg
    mean = grp[..., 0] / n
    var = (grp[..., 1] / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = rstd.repeat_interleave(cpg, 1) * gamma.double()[None]
    shift = beta.double()[None] - mean.repeat_interleave(cpg, 1) * scale
    return torch.stack([scale, shift], -1)


def fold_reference(st, S_out):
    B, S_in, C, _ = st.shape
    assert S_in % S_out == 0
    return st.double().view(B, S_out, S_in // S_out, C, 2).sum(2)


def softmax_reference(x, scale):
    return torch.softmax(x.double() * scale, dim=-1)


def group_errors(got, ref, lines_per_group=16):
    """rel-RMS of every group of `lines_per_group` adjacent lines of [outer, R, inner] tensors, and the maximum over the
    groups: one wrong group among thousands shows at full size.  -> ([outer, inner / lines_per_group] float64, float)"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape and got.ndim == 3, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    outer, R, inner = ref.shape
    assert inner % lines_per_group == 0
    sq = lambda t: t.pow(2).view(outer, R, inner // lines_per_group, lines_per_group).sum((1, 3))
    err = (sq(got - ref) / sq(ref).clamp_min(1e-300)).sqrt()
    return err, float(err.max())


def planes_as_lines(y):
    """NHWC [B, H, W, C] -> [B * H, W, C]: the lines of a W pass, so group_errors sees 16 channels of one pixel row"""
    B, H, W, C = y.shape
    return y.reshape(B * H, W, C)


# ------------------------------------------------------------------------------------------------ model of the roundings
def _bf(x):
    return x.float().to(torch.bfloat16).double()


def emulate_bf16(x, M, M2=None, act=0, table=None, C=0, outer_per_sample=1):
    """What a CORRECT bf16 k_sep computes, rounding for rounding (not its instruction order): M and M2 rounded to bf16, the
    products exact, xn (fp32 x * scale + shift) rounded to bf16 when the table is on, the SiLU output rounded to bf16 in
    the chained form, the result rounded to bf16.  float64 values that are bf16 numbers."""
    if table is None:
        xn = x.double()
    else:
        outer, K, inner = x.shape
        b = torch.arange(outer) // outer_per_sample
        c = torch.arange(inner) % C
        t = table.float()[b][:, c]
        xn = _bf(x.float() * t[:, None, :, 0] + t[:, None, :, 1])
    z = torch.einsum("rk,oki->ori", _bf(M), xn)
    if M2 is not None:
        return _bf(torch.einsum("sr,ori->osi", _bf(M2), _bf(silu64(z))))
    return _bf(silu64(z) if act else z)


# ------------------------------------------------------------------------------------------------ input recipes
def lines(outer, K, inner, dtype, seed=0):
    """N(0, 1) with per-line scales in [0.5, 1.5), per-sample-index scales in [0.75, 1.25) and a small per-line offset: no two
    lines, groups or positions along k are exchangeable, and nothing repeats with the period of a sweep."""
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.randn(outer, K, inner, generator=g)
    x *= 0.5 + torch.rand(1, 1, inner, generator=g)
    x *= 0.75 + 0.5 * torch.rand(1, K, 1, generator=g)
    x += 0.25 * torch.randn(1, 1, inner, generator=g)
    return rnd(x, dtype)


def planes(B, C, N, dtype, seed=0):
    """NCHW fp32 planes for the composed paths, per-channel scale and offset"""
    g = torch.Generator().manual_seed(3000 + seed)
    x = torch.randn(B, C, N, N, generator=g) * (0.5 + torch.rand(1, C, 1, 1, generator=g))
    x += 0.5 * torch.randn(B, C, 1, 1, generator=g)
    return rnd(x, dtype)


def gn_tables(B, C, seed=0):
    """[B, C, 2] fp32: scales of either sign with magnitude in [0.5, 1.5), shifts N(0, 0.5^2); distinct per sample and channel"""
    g = torch.Generator().manual_seed(4000 + seed)
    scale = (0.5 + torch.rand(B, C, generator=g)) * (1.0 - 2.0 * (torch.rand(B, C, generator=g) < 0.25).float())
    shift = 0.5 * torch.randn(B, C, generator=g)
    return torch.stack([scale, shift], -1).contiguous()


def affine(C, seed=0):
    g = torch.Generator().manual_seed(5000 + seed)
    return 1.0 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)


def partials(B, S, C, per_split, mean=0.0, std=1.0, seed=0):
    """GroupNorm partial sums as a producer leaves them: float64 data [B, S * per_split, C] with per-channel mean / std
    around (mean, std), summed per split in float64 and cast to fp32.  -> (st [B, S, C, 2] fp32, HW)"""
    g = torch.Generator().manual_seed(6000 + seed)
    x = torch.randn(B, S, per_split, C, generator=g, dtype=torch.float64)
    x = x * (std * (0.5 + torch.rand(1, 1, 1, C, generator=g, dtype=torch.float64)))
    x = x + mean + 0.5 * std * torch.randn(B, 1, 1, C, generator=g, dtype=torch.float64)
    st = torch.stack([x.sum(2), x.pow(2).sum(2)], -1)
    return st.float().contiguous(), S * per_split


def softmax_rows(cols, scale, dtype, seed=0):
    """Rows of logits (fp32, rounded through dtype) and their names: randn * 4; one logit 60 nats (after `scale`) above N(0, 1)
    rest at index 0 and at cols - 1; a constant row; fp32 only: randn * 4 offset by +3e4."""
    g = torch.Generator().manual_seed(7000 + seed + cols)
    rows, names = [torch.randn(cols, generator=g) * 4.0], ["randn*4"]
    for at in (0, cols - 1):
        r = torch.randn(cols, generator=g)
        r[at] = r[at] + 60.0 / scale
        rows.append(r)
        names.append(f"spike@{at}")
    rows.append(torch.full((cols,), 1.375))
    names.append("constant")
    if dtype == torch.float32:
        rows.append(torch.randn(cols, generator=g) * 4.0 + 3e4)
        names.append("offset+3e4")
    else:
        rows.append(torch.randn(cols, generator=g) * 4.0 - 2.0)
        names.append("randn*4-2")
    return rnd(torch.stack(rows), dtype), names


def sweep_checkpoints(n=SWEEP_GROUPS):
    """The groups of an n-group launch that are compared with float64: the first 512, the last 16, and 16 either side of every
    multiple of 1024 (a sweep of the grid is 1024 or 2048 groups)."""
    idx = set(range(512)) | set(range(n - 16, n))
    for edge in range(1024, n, 1024):
        idx |= set(range(edge - 16, min(edge + 16, n)))
    return sorted(idx)
