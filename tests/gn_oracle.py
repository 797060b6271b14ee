"""float64 oracle for the GroupNorm partial-sum format and everything that consumes it (importable on the CPU).

The format (GnStats in csrc/common.hpp, ops.GNStats): st[b][s][c] = (sum x, sum x^2) in fp32 of channel c over pixel split s of
sample b.  A producer writes it; every consumer adds, for group g, the partials of its channels over all splits of one or two
tensors (a virtual channel concat), finishes mean / rstd itself and applies y = x k + sh with k = rstd gamma, sh = beta - mean k.

Two kinds of data:
  hard_planes   every (sample, group) has its own mean (|mean| in [ratio / 2, ratio], either sign) and its own standard deviation
                in [0.5, 1.5], so reading the statistics of another sample, another group, or the other half of a concat moves the
                result by O(1) - O(ratio).  One group of one sample (const_key) is exactly constant, at a power of two v, so
                its partial sums are exact and its raw variance is exactly 0: `starved` lowers its sum of squares by one fp32
                step and the raw variance s2/n - m^2 turns slightly negative (-v^2 2^-24 .. -v^2 2^-23) - the fmaxf(var, 0)
                clamp has to act.  Two constants, because no single one serves both kinds of check: with rstd = eps^-1/2 the
                fp32 formula x k + sh carries u v eps^-1/2 of absolute error on that group whatever the kernel does, and an
                unclamped variance reaches -eps (NaN) only when v^2 u > eps - then that error is above sqrt(u) = 2.4e-4.
                  const = 0.25 (default, "quiet"): the error is 5e-6 at eps = 1e-5, inside the max-norm classes of close();
                          a missing clamp moves k by 4e-4, far outside gn_table's 4 u bound.
                  const = "loud": the power of two next below `ratio` (8, 32): a missing clamp is a NaN at ratio 32; only for
                          checks with the element-wise apply_bound, which prices the cancellation in.
  int_planes    integers in [-8, 8].  With HW * 64 < 2^24 every sum x and sum x^2 over any set of pixels is an integer below 2^24:
                an exact fp32 value in ANY order of addition, so a producer must equal `partials` bit for bit.

The reference of a CONSUMER is `finish` on the very partials the kernel is handed (summed in float64, variance clamped at 0)
followed by `apply` in float64.  Kernel and reference start from identical fp32 partials, so what is left is the kernel's own
arithmetic, bounded element-wise by `apply_bound`.

What the FORMAT itself loses against the true statistics of the data is a different matter and no kernel's fault: sum x^2 ~ n
mean^2 is rounded to fp32 per partial, and the variance (~ std^2) is what is left after subtracting mean^2.  Relative error of rstd
against float64 statistics of the same fp32 data (HW = 64, 8 channels per group, 4 splits, 3 x 4 (sample, group) keys; the worst
key, recorded by test_gn_oracle_host.test_format_rstd_error_table):

    ratio             0.5        8          32         128
    max rel. error    7.0e-9     1.1e-6     7.5e-6     1.7e-4      (it grows with ratio^2: about 1e-8 ratio^2)

so the end-to-end checks against true GroupNorm stay at ratio <= 8 (asserted <= 2e-6 there), and the consumer checks at ratio 32
use `finish` on the same partials.
"""
import torch

EPS24 = 2.0 ** -24
MAX_INT = 8
MAX_SUM = 1 << 24

# recorded by test_format_rstd_error_table (printed there; asserted only at ratio <= 8)
FORMAT_RSTD_ERR = {0.5: 7.0e-9, 8: 1.1e-6, 32: 7.5e-6, 128: 1.7e-4}


def const_key(B, G):
    """(sample, group) that hard_planes makes exactly constant."""
    return B // 2, G // 3


def _const_value(ratio):
    v = 1.0
    while v * 2 <= ratio:
        v *= 2
    while v > ratio:
        v /= 2
    return v


def hard_planes(B, C, G, HW, ratio, seed, dtype, const=0.25):
    """x [B, HW, C] fp32, rounded through `dtype`.  Group (b, g): mean = +-ratio * U[0.5, 1], std = U[0.5, 1.5] - of the group's
    own elements, not of a distribution: a group of two elements (HW = 1) must not come out with a deviation near 0, where
    rstd and with it the cancellation in x k + sh are anyone's guess - each channel with a further offset so that channels differ; group const_key(B, G) is the constant `const`
    ("loud": the power of two next below `ratio`; see the module docstring)."""
    assert C % G == 0
    gen = torch.Generator().manual_seed(seed)
    cpg = C // G
    sign = torch.randint(0, 2, (B, 1, G, 1), generator=gen).double() * 2 - 1
    mean = sign * ratio * (0.5 + 0.5 * torch.rand((B, 1, G, 1), generator=gen, dtype=torch.float64))
    std = 0.5 + torch.rand((B, 1, G, 1), generator=gen, dtype=torch.float64)
    off = 0.25 * torch.randn((B, 1, G, cpg), generator=gen, dtype=torch.float64)
    z = torch.randn((B, HW, G, cpg), generator=gen, dtype=torch.float64) + off
    if HW * cpg > 1:                                           # the SAMPLE deviation of every group is `std`, also for 2 elements
        z = (z - z.mean((1, 3), keepdim=True)) / z.var((1, 3), unbiased=False, keepdim=True).sqrt()
    x = mean + std * z
    b, g = const_key(B, G)
    x[b, :, g, :] = _const_value(ratio) if const == "loud" else const
    return x.view(B, HW, C).to(dtype).to(torch.float32)


def int_planes(B, C, HW, seed, dtype):
    """x [B, HW, C] fp32 of integers in [-8, 8] (bf16 values): exact partial sums in any order.  The cap is a condition."""
    assert HW * MAX_INT * MAX_INT < MAX_SUM, f"HW = {HW}: sum x^2 can reach 2^24, not an exact case"
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-MAX_INT, MAX_INT + 1, (B, HW, C), generator=gen).float()
    y = x.to(dtype).to(torch.float32)
    assert torch.equal(x, y)
    return y


def even_cuts(HW, S):
    """The split boundaries of the stand-alone producer: cuts[s] = HW * s // S."""
    return [HW * s // S for s in range(S + 1)]


def ragged_cuts(HW, S, seed):
    """S splits of unequal length (empty ones included when they must or may be): a sorted draw of S - 1 interior boundaries
    below HW, so that the LAST split always holds a pixel - the one a consumer's tail loop (S % 8) must not lose."""
    gen = torch.Generator().manual_seed(seed)
    inner = sorted(int(v) for v in torch.randint(0, HW, (S - 1,), generator=gen))
    return [0] + inner + [HW]


def partials(x, cuts):
    """fp32 [B, S, C, 2] partial sums of x [B, HW, C] over the pixel ranges [cuts[s], cuts[s + 1]): summed in float64, rounded
    once (exact for int_planes)."""
    B, HW, C = x.shape
    assert cuts[0] == 0 and cuts[-1] == HW and all(a <= b for a, b in zip(cuts, cuts[1:]))
    xd = x.double()
    out = torch.zeros((B, len(cuts) - 1, C, 2), dtype=torch.float64)
    for s, (p0, p1) in enumerate(zip(cuts, cuts[1:])):
        out[:, s, :, 0] = xd[:, p0:p1].sum(1)
        out[:, s, :, 1] = (xd[:, p0:p1] ** 2).sum(1)
    return out.float()


def starved(st, G, C=None, c_off=0):
    """The partials `st` (channels [c_off, c_off + Cs) of a C-channel concat) with every non-zero sum of squares of the constant
    group's channels one fp32 step lower."""
    B, _, Cs, _ = st.shape
    C = Cs if C is None else C
    cpg = C // G
    b, g = const_key(B, G)
    lo, hi = max(g * cpg - c_off, 0), min((g + 1) * cpg - c_off, Cs)
    out = st.clone()
    if hi > lo:
        s2 = out[b, :, lo:hi, 1]
        out[b, :, lo:hi, 1] = torch.where(s2 > 0, torch.nextafter(s2, torch.zeros_like(s2)), s2)
    return out


def group_sums(st1, st2, G):
    """float64 [B, G, 2] (sum x, sum x^2) per group from the fp32 partials of one tensor or of a concat."""
    s = st1.double().sum(1)
    if st2 is not None:
        s = torch.cat([s, st2.double().sum(1)], 1)
    B, C, _ = s.shape
    return s.view(B, G, C // G, 2).sum(2)


def finish(st1, st2, G, n, eps):
    """float64 (mean, rstd) [B, G]: the given fp32 partials summed in float64, variance clamped at 0.  n = HW * C / G."""
    s = group_sums(st1, st2, G)
    mean = s[..., 0] / n
    var = (s[..., 1] / n - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + eps)


def scale_shift(mean, rstd, gamma, beta, G):
    """float64 per-channel (k, sh) [B, C]: k = rstd gamma, sh = beta - mean k."""
    C = gamma.numel()
    k = rstd.repeat_interleave(C // G, 1) * gamma.double()
    sh = beta.double() - mean.repeat_interleave(C // G, 1) * k
    return k, sh


def apply(x, mean, rstd, gamma, beta, G):
    """float64 GroupNorm-apply of x [B, ..., C] with the given (mean, rstd) [B, G]."""
    k, sh = scale_shift(mean, rstd, gamma, beta, G)
    shape = (x.shape[0],) + (1,) * (x.dim() - 2) + (x.shape[-1],)
    return x.double() * k.view(shape) + sh.view(shape)


def apply_bound(x, k, sh, ref, dtype=torch.float32):
    """Element-wise bound on |kernel - ref| for act = 0.  The kernel computes in fp32 (u = 2^-24: one rounding is <= u relatively)
        var32 = fl(var), rstd' = rsqrtf(fl(var32 + eps)), k' = fl(rstd' gamma), sh' = fl(beta - fl(fl(mean) k')), y = fl(fl(x k') + sh')
    from the same partials as the reference, summed in fp64 on both sides, so mean and var start out equal.
      rstd': u in var32 and u in the sum with eps are u / 2 each in the root; rsqrtf is good to 1 ulp = 2u: rstd (1 + 3u).
      k':    one more rounding: k (1 + d), |d| <= 4u.
      x k':  d |x k| + u |x k| (the product; absent where the compiler contracts the line into an fma).
      sh':   d |mean k| + 2u |mean k| (fl(mean), the product) + u |sh| (the subtraction).
      y:     u |ref| (the sum).
    The two d terms are the SAME relative error of k' with opposite signs: together d (x - mean) k = d (ref - beta), at most
    4u (|ref| + |beta|).  First order in all: u |x k| + 2u |mean k| + u |sh| + 5u |ref| + 4u |beta|, and with |mean k| <= |sh| +
    |beta|: u |x k| + 3u |sh| + 5u |ref| + 6u |beta|.  8u (|x k| + |sh| + |ref|) covers that with a factor of about 2 to spare
    wherever |beta| does not exceed |x k| + |sh| + |ref| by much - everywhere but at an element with x ~ 0 in a channel whose
    beta happens to equal mean k, which random gamma / beta against |mean| >= ratio / 2 do not produce.  An fp32 emulation of the
    formula stays within 0.64 of the bound up to ratio 128 (test_gn_oracle_host prints it), the kernel within 0.18 (fp32).
    A bf16 result is rounded to nearest once more when stored: bf16 keeps 8 significant bits, half an ulp is at most 2^-8 |ref|."""
    shape = (x.shape[0],) + (1,) * (x.dim() - 2) + (x.shape[-1],)
    bound = 8 * EPS24 * ((x.double() * k.view(shape)).abs() + sh.view(shape).abs() + ref.abs())
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    return bound


def true_groupnorm(x, gamma, beta, G, eps):
    """float64 GroupNorm of x [B, HW, C] from the data itself (two-pass statistics)."""
    B, HW, C = x.shape
    xg = x.double().view(B, HW, G, C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, G, 1)) ** 2).mean((1, 3))
    return apply(x, mean, 1.0 / torch.sqrt(var + eps), gamma, beta, G)
