"""Addressed inputs for the fused attention block (csrc/attnf.hip) and the fused UNet tail (csrc/convout.hip): importable on the CPU.

Both kernels carry a GroupNorm, and a softmax or a SiLU, inside the launch, so the bit-for-bit oracle of tests/exact_oracle.py
does not reach them, and on random data their tests can only bound a relative RMS error over the whole tensor - which a fault
confined to one key, one row or one border pixel passes.  Here the inputs are built so that a plain float64 evaluation of the
same operation does not move under any legitimate rounding but moves by O(1) under any wrong index:

  * the GroupNorm partial sums are fabricated (as tests/test_gpu_groupnorm_stats.Case does): every (sample, group) reports an
    integer mean m[b, g] and a variance of exactly 0.5, and the call passes eps = 0.5.  The kernel's finish is then
    rstd = rsqrtf(1.0f) and mean = m, the scale is gamma_c and the shift beta_c - m gamma_c: small integers.  Everything the
    kernels form from the scale is rounded to bf16 before use (attnf.hip: W' = bf16(W a); convout.hip: bf16(silu(x k + sh))),
    so an ulp in rstd cannot change a bit as long as the products are integers of at most 8 significant bits;
  * attention: n = log2 T code channels of the normalised tokens hold the +-1 binary code of (token XOR a per-sample scramble);
    to_k copies the code, to_q copies a per-head bit permutation of it with per-head signs, both with an amplitude that puts
    tens of log2 units between the one key whose code matches and every other key: query i of head h returns row pi_h(i) of
    v, a bijection that differs per head and crosses the 32-token tiles.  Two more recipes give every key equal weight
    ("uniform": to_q = 0) and the T / 4 keys that match in two code bits equal weight ("subset");
  * the tail: normalised values come from {0, 8, 16, 24, 32} - where bf16(silu(v)) = v - and {-256, -128}, where silu_f
    returns -0; weights are ternary and the bias a multiple of 8, so the float64 result is a bf16 value and the kernel must
    EQUAL it.

The conditions that make this so are asserted on the reference (check_attention_case, tail_case), never on a kernel's output: a
case that breaks one gets another seed or amplitude, not a wider bound.
"""
import math
import types

import torch
import torch.nn.functional as F

import exact_oracle as xo
import gn_oracle as go

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634
VAR = 0.5                  # the variance every (sample, group) reports ...
EPS = 0.5                  # ... and the eps the call passes: var + eps = 1
SPLITS = (1, 3, 9)         # split counts of the fabricated partials (gn_channel_sums: tail only, 8 + 1; attnf.hip: cpg x S walk)
TILE = 32                  # tokens of one query / key tile of k_attn_fused
MASS_CAP = 2.0 ** -10      # condition (ii): 4 (1 - p_in) max|v| stays below this

# every shape afldm_attn_block_fused_supported admits (T is fixed by the kernels: these are the smallest shapes)
SHAPES = [(1024, 192, 8), (256, 384, 16), (256, 64, 4), (64, 128, 8)]
RECIPES = ("addressed", "uniform", "subset")
# (to_q, to_k) amplitudes.  8 / 8: the gap between the target and the next key is 2 * 64 * scale * log2 e = 37.7 log2 units at
# head_dim 24, 46.2 at 16.  T = 64: the first key tile is half of all keys, every target is within one bit of it and no wave
# would ever leave the bounded loop (limit 80); 16 / 8 makes one bit 92.3 units
AMPLITUDES = {64: (16, 8)}
# the "subset" recipe, by head_dim: SMALL scores - a gap of 2 aq ak scale log2 e = 21.2 (head_dim 24) / 23.1 (16) log2 units between the
# T / 4 matching keys and the rest, so that every wave stays in the bounded loop and 1 - p_in (about 2 * 2^-gap) stays ABOVE 2^-24:
# where the mean over the matching keys cancels to zero the tolerance is its mass term alone, and that has to cover one fp32 unit of
# the addends.  (With the 16 / 8 amplitudes at T = 64 the gap is 92 units, the mass term 4e-26, and the MI355X stores -2^-24 where
# the float64 mean is -1e-28: the row-maxima loop rescales the first tile's sum to -1e-26, and the MFMA that adds the 16 matching
# products +-P v - they cancel exactly - aligns that remainder to the largest product and truncates it to one unit of its adder,
# -2^-20, over a row sum of 16.  An fp32-sized error on addends of size 16: legitimate, and the case's fault, not the kernel's.)
SUBSET_AMPLITUDES = {24: (6, 6), 16: (8, 4)}
FP32_UNIT = 2.0 ** -24
# query tiles per attention pass of the instantiation that runs the shape (AttnFCfg::NU): a wave chooses its loop over all of them
TILES_PER_PASS = {(1024, 24): 2, (256, 24): 2, (256, 16): 1, (64, 16): 1}
BOUNDED_LIMIT = 80.0


def is_bf16(t):
    return torch.equal(t.to(BF16).to(t.dtype), t)


def is_int8bit(t):
    """Integers of at most 8 significant bits: bf16 values that a relative error of an ulp of fp32 cannot move to another."""
    return torch.equal(t, t.round()) and is_bf16(t)


# ------------------------------------------------------------------------------------------------ a. GroupNorm partials
def group_means(B, G, seed=0):
    """Integer means in [-3, 3], different between neighbouring samples (step 2 mod 7) and groups (step 3 mod 7).  [B, G] float64"""
    b, g = torch.arange(B)[:, None], torch.arange(G)[None, :]
    return ((2 * b + 3 * g + seed) % 7 - 3).double()


def partials(m, C, HW, S, seed=0):
    """fp32 [B, S, C, 2]: per channel s1 = HW m and s2 = HW (m^2 + 0.5), cut into S ragged runs of pixels (three different cuts,
    by channel % 3; empty runs included) - integers and half-integers, exact in fp32.  The float64 finish of exactly these gives
    mean = m and rstd = 1: asserted."""
    B, G = m.shape
    mc = m.repeat_interleave(C // G, 1)                                                        # [B, C]
    st = torch.zeros(B, S, C, 2, dtype=torch.float64)
    for r in range(3):
        cuts = go.ragged_cuts(HW, S, 1000 * seed + 31 * S + 7 * r + HW)
        n = torch.tensor([b - a for a, b in zip(cuts, cuts[1:])], dtype=torch.float64)[None, :, None]
        ch = torch.arange(r, C, 3)
        st[:, :, ch, 0] = n * mc[:, None, ch]
        st[:, :, ch, 1] = n * (mc[:, None, ch] ** 2 + VAR)
    out = st.float()
    assert torch.equal(out.double(), st), "the partials are not fp32 values"
    mean, rstd = go.finish(out, None, G, HW * (C // G), EPS)
    assert torch.equal(mean, m) and torch.equal(rstd, torch.ones_like(rstd)), "the finish of the partials is not (m, 1)"
    return out


def _choice(values, shape, gen):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=gen)]


# ------------------------------------------------------------------------------------------------ b. attention
def code_bits(tok, n):
    """+-1 binary code of integer tokens: [..., n], bit r -> +1 where set."""
    return (((tok[..., None] >> torch.arange(n)) & 1) * 2 - 1).double()


def attention_case(B, T, C, heads, recipe, seed=0, G=32, amplitude=None):
    """Operands (float64 CPU tensors of small integers) of one attention block:
      x [B, T, C] raw tokens, m [B, G], gamma / beta [C], h [B, T, C] the normalised tokens gamma (x - m) + beta,
      wq / wk / wv [C, C], bq / bk / bv [C], scale = head_dim^-0.5, scramble [B], code_ch [n]."""
    assert recipe in RECIPES and T == 1 << int(math.log2(T)) and C % heads == 0 and C % G == 0
    n, d, cpg = int(math.log2(T)), C // heads, C // G
    assert n <= d
    aq, ak = amplitude or (SUBSET_AMPLITUDES[d] if recipe == "subset" else AMPLITUDES.get(T, (8, 8)))
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * T + 31 * C + heads + 131 * B)
    c = types.SimpleNamespace(B=B, T=T, C=C, heads=heads, G=G, d=d, n=n, recipe=recipe, seed=seed, amplitude=(aq, ak), scale=d ** -0.5)
    c.m = group_means(B, G, seed)
    c.gamma, c.beta = _choice([1, 2, -1], (C,), gen), _choice([-1, 0, 1], (C,), gen)
    c.code_ch = torch.round(torch.linspace(0, C - 1, n)).long()                                # spread over the whole channel range
    assert c.code_ch.unique().numel() == n
    even = (c.gamma[c.code_ch] == 2) & (c.beta[c.code_ch] == 0)                                # h = +-1 = 2 u + beta needs an odd beta
    c.beta[c.code_ch[even]] = 1.0
    # a scramble per sample, all different, none zero
    c.scramble = (torch.randperm(T - 1, generator=gen)[:B] + 1).long()
    code = code_bits(torch.arange(T)[None, :] ^ c.scramble[:, None], n)                         # [B, T, n]
    # the other channels: integers in [-2, 2] of the form gamma u + beta
    h0 = torch.randint(-2, 3, (B, T, C), generator=gen).double()
    u = torch.div(h0 - c.beta, c.gamma, rounding_mode="trunc")
    u[:, :, c.code_ch] = (code - c.beta[c.code_ch]) / c.gamma[c.code_ch]
    c.h = c.gamma * u + c.beta
    assert torch.equal(u, u.round()) and float(c.h.abs().max()) <= 2 and torch.equal(c.h[:, :, c.code_ch], code)
    c.x = c.m.repeat_interleave(cpg, 1)[:, None, :] + u
    # projections
    c.wv, c.bv = xo.ternary((C, C), 0.25, gen).double(), xo.small_ints((C,), -4, 4, gen).double()
    c.wq, c.wk = torch.zeros(C, C, dtype=torch.float64), torch.zeros(C, C, dtype=torch.float64)
    c.bq, c.bk = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    kbits = list(range(n)) if recipe != "subset" else [n - 1, n - 2]                           # subset: two HIGH bits
    c.rho, c.mask = [], []
    for hd in range(heads):
        rot = 1 + hd % (n - 1)                                                                 # never the identity: targets leave their tile
        mask = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
        c.rho.append(rot)
        c.mask.append(mask)
        for r, kb in enumerate(kbits):
            c.wk[hd * d + r, c.code_ch[kb]] = ak
            if recipe != "uniform":
                c.wq[hd * d + r, c.code_ch[(kb + rot) % n]] = aq * float(mask[kb])
    keys = [(r, tuple(mk.tolist())) for r, mk in zip(c.rho, c.mask)]
    assert len(set(keys)) == heads, "two heads address alike: another seed"
    c.what = f"{recipe} B{B} T{T} C{C} heads{heads} seed{seed}"
    return c


def attention_reference(c, w_out=None, b_out=None):
    """Plain float64 softmax(q k^T scale) v on the integer q, k, v of the case, sample by sample.  Fills
      c.v [B, T, C], c.ref [B, T, C], c.off [B, heads, T] = 1 - p_in (the softmax mass OFF the keys that attain the row maximum,
      summed directly), c.target [B, heads, T] (a key that attains the maximum), c.hits [B, heads, T] (how many do)."""
    B, T, C, heads, d = c.B, c.T, c.C, c.heads, c.d
    q = (c.h @ c.wq.T + c.bq).view(B, T, heads, d).transpose(1, 2)
    k = (c.h @ c.wk.T + c.bk).view(B, T, heads, d).transpose(1, 2)
    c.v = c.h @ c.wv.T + c.bv
    v = c.v.view(B, T, heads, d).transpose(1, 2)
    c.q_int, c.k_int = q, k
    ref, off, target, hits = [], [], [], []
    for b in range(B):
        s = q[b] @ k[b].transpose(1, 2) * c.scale                                              # [heads, T, T], nats
        p = torch.softmax(s, -1)
        top = s == s.max(-1, keepdim=True).values
        ref.append(p @ v[b])
        off.append((p * ~top).sum(-1))
        target.append(s.argmax(-1))
        hits.append(top.sum(-1))
    c.ref = torch.stack(ref).transpose(1, 2).reshape(B, T, C)
    c.off, c.target, c.hits = torch.stack(off), torch.stack(target), torch.stack(hits)
    c.vmax = float(c.v.abs().max())
    c.tol = tolerance(c.ref, c.off, c.vmax, heads)
    return c


def tolerance(ref, off, vmax, heads):
    """tol = 2^-8 |ref| + 4 (1 - p_in) max|v|, per element.  The first term is one bf16 ulp of the stored value.  The second is the
    mass outside the maximal keys, doubled once because the bf16 rounding of q scale log2 e moves a score by less than one log2
    unit (asserted by check_attention_case) and once because that mass enters numerator and denominator.  The kernel rounds P to
    bf16 and takes its row sums from the same rounded P: that rounding cancels (P is equal on all maximal keys)."""
    B, T, C = ref.shape
    mass = (4.0 * off * vmax).transpose(1, 2)[..., None].expand(B, T, heads, C // heads).reshape(B, T, C)
    return 2.0 ** -8 * ref.abs() + mass


def check_attention_case(c):
    """The conditions of the design, on the operands and the float64 reference alone."""
    B, T, C, heads, d = c.B, c.T, c.C, c.heads, c.d
    for name in ("x", "h", "gamma", "beta", "wq", "wk", "wv", "bq", "bk", "bv"):
        assert is_int8bit(getattr(c, name)), f"{c.what}: {name} is not made of small integers"
    # what the kernel forms from the scale: W' = bf16(W gamma rstd), and the three-launch path's bf16(gamma (x - m) rstd + beta)
    for name in ("wq", "wk", "wv"):
        assert is_int8bit(getattr(c, name) * c.gamma), f"{c.what}: gamma {name} is not exact in bf16"
    assert is_int8bit(c.q_int) and is_int8bit(c.k_int) and float(c.q_int.abs().max()) <= 256
    # (iii) v is stored unchanged, and the rows of distinct tokens differ in every head
    assert c.vmax <= xo.MAX_ABS and is_int8bit(c.v), f"{c.what}: max|v| = {c.vmax}"
    vh = c.v.view(B, T, heads, d)
    for b in range(B):
        for hd in range(heads):
            assert torch.unique(vh[b, :, hd], dim=0).shape[0] == T, f"{c.what}: two tokens share a v row in head {hd}: another seed"
    # (i) which keys attain the maximum
    if c.recipe == "addressed":
        assert int(c.hits.max()) == 1
        assert torch.equal(c.target.sort(-1).values, torch.arange(T).expand(B, heads, T)), f"{c.what}: the targets are no bijection"
        tq, tk = torch.arange(T) // TILE, c.target // TILE
        assert bool((tq != tk).any(-1).all()), f"{c.what}: a head keeps every query inside its own key tile"
        for hd in range(1, heads):
            assert not torch.equal(c.target[:, hd], c.target[:, 0]), f"{c.what}: heads 0 and {hd} address alike"
        for b in range(1, B):
            assert not torch.equal(c.target[b], c.target[0]), f"{c.what}: samples 0 and {b} address alike"
    else:
        assert bool((c.hits == (T if c.recipe == "uniform" else T // 4)).all()), f"{c.what}: {c.hits.unique().tolist()} maximal keys"
    # (ii) the mass term of the tolerance is negligible
    assert 4.0 * float(c.off.max()) * c.vmax <= MASS_CAP, f"{c.what}: 4 (1 - p_in) max|v| = {4.0 * float(c.off.max()) * c.vmax:.3e}"
    # (v) where a mean over several keys can cancel to zero, the mass term covers an fp32 unit of the addends (see SUBSET_AMPLITUDES;
    # the uniform recipe has no mass term and needs none: every product and partial sum there is an integer)
    if c.recipe == "subset":
        assert float(c.off.min()) >= FP32_UNIT, f"{c.what}: 1 - p_in = {float(c.off.min()):.3e} < 2^-24: a lower amplitude"
    # the bf16 rounding of q scale log2 e moves no score by a log2 unit
    qs = torch.tensor(c.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qb = (c.q_int.float() * qs).to(BF16).double()
    c.score_shift = float(((qb - c.q_int * c.scale * LOG2E).abs() * c.k_int.abs().amax(2, keepdim=True)).sum(-1).max())
    assert c.score_shift < 1.0, f"{c.what}: the rounding of q moves a score by {c.score_shift:.3f} log2 units"
    return c


_CASES = {}


def cached_attention_case(B, T, C, heads, recipe, seed=0):
    """attention_case + attention_reference + check_attention_case, built once per process and left unchanged."""
    key = (B, T, C, heads, recipe, seed)
    if key not in _CASES:
        _CASES[key] = check_attention_case(attention_reference(attention_case(B, T, C, heads, recipe, seed)))
    return _CASES[key]


def to_out_case(c, seed=0):
    """A ternary to_out with an integer bias for the case: y = to_out(o) + x in float64 from the float64 o, and its tolerance - one
    bf16 ulp of y plus the tolerance of o (the bf16 store of o, the mass term) carried through the sum of |w_out|.
    (iv): max|y| <= 256; where o is integral (the addressed recipe) all caps of exact_oracle.check_caps."""
    gen = torch.Generator().manual_seed(4099 * seed + c.T + c.C + 17)
    c.wo, c.bo = xo.ternary((c.C, c.C), 1.0 / 16, gen).double(), xo.small_ints((c.C,), -4, 4, gen).double()
    c.y = c.ref @ c.wo.T + c.bo + c.x
    c.y_tol = 2.0 ** -8 * c.y.abs() + c.tol @ c.wo.abs().T
    c.y_int = None
    if c.recipe == "addressed":                    # o is the integer row v[pi(i)] up to the mass term: y of that row is what a kernel stores
        c.y_int = c.ref.round() @ c.wo.T + c.bo + c.x
        xo.check_caps(c.y_int, c.what + " y")
        assert bool(((c.y - c.y_int).abs() <= c.y_tol).all())
    assert float(c.y.abs().max()) <= xo.MAX_ABS, f"{c.what}: max|y| = {float(c.y.abs().max())}"
    return c


def over_tolerance(got, ref, tol):
    """Boolean mask of the elements outside the tolerance (a NaN is outside)."""
    g = torch.as_tensor(got).detach().double().cpu()
    assert g.shape == ref.shape, f"shape {tuple(g.shape)} != {tuple(ref.shape)}"
    return ~((g - ref).abs() <= tol)


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over the elements with a positive tolerance; elsewhere (ref = 0 and no mass: tol = 0) a difference
    counts as infinite."""
    g = torch.as_tensor(got).detach().double().cpu()
    diff = (g - ref).abs()
    r = torch.where(tol > 0, diff / tol.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def assert_addressed(got, c, what="", ref=None, tol=None):
    """Every element of got [B, T, C] within the case's tolerance of its float64 reference; on failure the count and the first
    (sample, head, token, channel) offenders with the token whose v row the reference returns there.  Returns the worst
    |got - ref| / tol."""
    ref = c.ref if ref is None else ref
    tol = c.tol if tol is None else tol
    bad = over_tolerance(got, ref, tol)
    if not bool(bad.any()):
        return worst_ratio(got, ref, tol)
    g = torch.as_tensor(got).detach().double().cpu()
    idx = bad.nonzero()
    first = []
    for b, t, ch in idx[:8].tolist():
        hd = ch // c.d
        src = f"v row of token {int(c.target[b, hd, t])}" if c.recipe == "addressed" else f"mean over {int(c.hits[b, hd, t])} keys"
        first.append(f"(b {b}, head {hd}, token {t}, channel {ch}): got {float(g[b, t, ch]):g} want {float(ref[b, t, ch]):g} ({src})")
    spans = ", ".join(f"{n} in [{int(idx[:, i].min())}, {int(idx[:, i].max())}]" for i, n in enumerate(("b", "token", "channel")))
    raise AssertionError(f"{what} {c.what}: {idx.shape[0]} of {g.numel()} values outside the tolerance ({spans}); first: " + "; ".join(first))


# ------------------------------------------------------------------------------------------------ the kernel's rounding points
def emulated_kernel(c):
    """CPU model of k_attn_fused's roundings on the case: q scale log2 e rounded to bf16, k in bf16, scores and exp2 in fp32 against
    a bf16 reference maximum, P rounded to bf16, row sums from the rounded P, fp32 products, one bf16 store.  [B, T, C] float64"""
    qs = torch.tensor(c.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qb = (c.q_int.float() * qs).to(BF16).double()
    kb = c.k_int.to(BF16).double()
    vb = c.v.to(BF16).double().view(c.B, c.T, c.heads, c.d).transpose(1, 2)
    out = []
    for b in range(c.B):
        s = (qb[b] @ kb[b].transpose(1, 2)).float()
        m = s.max(-1, keepdim=True).values.to(BF16).float()
        p = torch.exp2(s - m).to(BF16).double()
        o = ((p @ vb[b]).float() / p.sum(-1, keepdim=True).float()).to(BF16)
        out.append(o.double())
    return torch.stack(out).transpose(1, 2).reshape(c.B, c.T, c.C)


def loops_taken(c, gaps):
    """gaps [B, heads, T / 32]: the kernel's predicate per query tile (tests/test_gpu_attention_edges._bounded_loop_gaps).  A wave
    takes the bounded loop when it holds for every query tile of its pass.  -> bool [B, heads, passes]: True = bounded loop."""
    nu = TILES_PER_PASS[(c.T, c.d)]
    per_pass = gaps.view(c.B, c.heads, -1, nu).max(-1).values
    assert float((per_pass - BOUNDED_LIMIT).abs().min()) >= 3.0, f"{c.what}: a tile sits within 3 log2 units of the limit"
    return per_pass <= BOUNDED_LIMIT


# ------------------------------------------------------------------------------------------------ d. planted faults
FAULTS = ["drop_key", "drop_tile", "swap_v_rows", "rowsum_misses_key", "rotate_query_tile", "other_head_to_v", "other_sample_partials"]


def block_operands(c):
    """The case as restated_block takes it: GroupNorm by (mean, rstd) [B, G]."""
    return types.SimpleNamespace(x=c.x, mean=c.m, rstd=torch.ones_like(c.m), gamma=c.gamma, beta=c.beta, wq=c.wq, wk=c.wk, wv=c.wv,
                                 bq=c.bq, bk=c.bk, bv=c.bv, heads=c.heads, scale=c.scale)


def restated_block(o, fault=None):
    """GroupNorm-apply -> to_q | to_k | to_v -> softmax attention in float64 on any operands, written out with an explicit key
    mask, numerator and row sum, and one fault planted in sample 1 / the last head (the faults a tile-boundary off-by-one makes):
      drop_key              the last key is never visited
      drop_tile             the last 32-key tile but one is never visited
      swap_v_rows           V rows 31 and 32 (either side of a tile boundary) change places
      rowsum_misses_key     the last key enters the numerator but not the row sum
      rotate_query_tile     the 32 output rows of query tile 1 are rotated by one
      other_head_to_v       the head's v is projected with the rows of head 0
      other_sample_partials sample 1 is normalised with the statistics of sample 0"""
    assert fault is None or fault in FAULTS
    B, T, C = o.x.shape
    heads, d, cpg = o.heads, C // o.heads, C // o.mean.shape[1]
    b0, h0 = 1, heads - 1
    mean, rstd = o.mean.double().clone(), o.rstd.double().clone()
    if fault == "other_sample_partials":
        mean[b0], rstd[b0] = mean[0], rstd[0]
    k_ = rstd.repeat_interleave(cpg, 1) * o.gamma.double()
    h = (o.x.double() - mean.repeat_interleave(cpg, 1)[:, None]) * k_[:, None] + o.beta.double()
    wv, bv = o.wv.double(), o.bv.double()
    if fault == "other_head_to_v":
        wv, bv = wv.clone(), bv.clone()
        wv[h0 * d:(h0 + 1) * d], bv[h0 * d:(h0 + 1) * d] = wv[:d].clone(), bv[:d].clone()
    q = (h @ o.wq.double().T + o.bq.double()).view(B, T, heads, d).transpose(1, 2)
    k = (h @ o.wk.double().T + o.bk.double()).view(B, T, heads, d).transpose(1, 2)
    v = (h @ wv.T + bv).view(B, T, heads, d).transpose(1, 2).clone()
    if fault == "swap_v_rows":
        v[b0, h0, [TILE - 1, TILE]] = v[b0, h0, [TILE, TILE - 1]]
    out = []
    for b in range(B):
        s = q[b] @ k[b].transpose(1, 2) * o.scale
        keep = torch.ones(heads, 1, T, dtype=torch.bool)
        if b == b0 and fault == "drop_key":
            keep[h0, :, T - 1] = False
        if b == b0 and fault == "drop_tile":
            keep[h0, :, T - 2 * TILE:T - TILE] = False
        s = s.masked_fill(~keep, float("-inf"))
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        num, den = e @ v[b], e.sum(-1, keepdim=True)
        if b == b0 and fault == "rowsum_misses_key":
            den[h0] = den[h0] - e[h0, :, T - 1:]
        ob = num / den
        if b == b0 and fault == "rotate_query_tile":
            ob[h0, TILE:2 * TILE] = ob[h0, TILE:2 * TILE].roll(1, 0)
        out.append(ob)
    return torch.stack(out).transpose(1, 2).reshape(B, T, C)


def random_block(T=1024, C=192, heads=8, B=2, G=32, eps=1e-5, hot=1.0):
    """The random recipe of test_attn_block_fused_vs_three_launch_path_and_reference (bf16-rounded operands, the statistics of the
    data itself) as restated_block operands: what the rel-RMS bounds of the existing tests see of the planted faults."""
    gen = torch.Generator().manual_seed(T + C)
    x = (torch.randn(B, T, C, generator=gen) * (1.0 + torch.rand(1, 1, C, generator=gen)) + 0.5 * torch.randn(1, 1, C, generator=gen))
    gamma, beta = 0.5 + torch.rand(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
    ws = [torch.randn(C, C, generator=gen) / C ** 0.5 for _ in range(3)]
    ws[0], ws[1] = ws[0] * hot, ws[1] * hot
    bs = [0.2 * torch.randn(C, generator=gen) for _ in range(3)]
    xb = x.to(BF16).double()
    wb = [w.to(BF16).double() for w in ws]
    xg = xb.view(B, T, G, C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, G, 1)) ** 2).mean((1, 3))
    return types.SimpleNamespace(x=xb, mean=mean, rstd=1.0 / torch.sqrt(var + eps), gamma=gamma, beta=beta, wq=wb[0], wk=wb[1], wv=wb[2],
                                 bq=bs[0], bk=bs[1], bv=bs[2], heads=heads, scale=(C // heads) ** -0.5)


def rel_rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ e. the UNet tail
TAIL_CLASSES = [(8, 16), (16, 16), (-16, 16), (128, -128)]          # (gamma, beta) of a channel
TAIL_IDENTITY = (0.0, 8.0, 16.0, 24.0, 32.0)                         # normalised values with bf16(silu(v)) = v (0: silu(0) = 0) ...
TAIL_ZERO = (-128.0, -256.0)                                        # ... and with silu_f(v) = -0: exp2 overflows, rcp(inf) = 0
TAIL_K_TERMS = 600                                                  # weight density min(0.5, 600 / K): sigma(y) <= 400, max|y| <= 2048
TAIL_B = 3


def tail_grid(C):
    """(Cout, G) of the conv_out_fused cases at C channels."""
    return [(Cout, G) for Cout in (1, 2, 3, 4) for G in (16, 32, 64) if C % G == 0]


def expected_silu_bf16(v):
    """What the kernel must store for a normalised value of the allowed set."""
    return torch.where(v > 0, v, torch.zeros_like(v))


def tail_case(B, C, Cout, G, seed=0, N=32):
    """conv_norm_out -> SiLU -> conv_out (3 x 3, C -> Cout) on x = m[b, g] + u, u ternary at density 0.5, with the channel classes
    TAIL_CLASSES: the activated tensor is made of 0, 8, 16, 24 and 32, the weights are ternary, the bias a multiple of 8 in
    [-64, 64], and y / 8 meets the caps of exact_oracle.check_caps.  With a positive shift on three channels in four, a kernel
    that activated its zero padding is off by >= 8 per live weight on every border pixel.
      x [B, N, N, C], m [B, G], gamma / beta [C], w [Cout, 3, 3, C] (OHWI), bias [Cout], act [B, N, N, C], ref [B, N, N, Cout] float64"""
    assert C % G == 0
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * C + 31 * Cout + G + 131 * B)
    c = types.SimpleNamespace(B=B, C=C, Cout=Cout, G=G, N=N, seed=seed)
    c.m = group_means(B, G, seed)
    cls = torch.randint(0, len(TAIL_CLASSES), (C,), generator=gen)
    table = torch.tensor(TAIL_CLASSES, dtype=torch.float64)
    c.gamma, c.beta = table[cls, 0], table[cls, 1]
    u = xo.ternary((B, N, N, C), 0.5, gen).double()
    c.x = c.m.repeat_interleave(C // G, 1)[:, None, None, :] + u
    c.norm = c.gamma * u + c.beta
    allowed = torch.tensor(TAIL_IDENTITY + TAIL_ZERO, dtype=torch.float64)
    assert bool(torch.isin(c.norm, allowed).all()), "a normalised value outside the allowed set"
    assert is_int8bit(c.x) and is_int8bit(c.gamma) and is_int8bit(c.beta) and is_int8bit(c.m.repeat_interleave(C // G, 1) * c.gamma)
    c.act = expected_silu_bf16(c.norm)
    K = 9 * C
    c.w_density = min(0.5, TAIL_K_TERMS / K)
    c.w = xo.ternary((Cout, 3, 3, C), c.w_density, gen)
    c.bias = 8.0 * xo.small_ints((Cout,), -8, 8, gen)
    c.ref = tail_reference(c.act, c.w, c.bias)
    c.what = f"conv_out_fused B{B} C{C}->{Cout} G{G} seed{seed}"
    c.max_abs, c.max_sumsq = xo.check_caps(c.ref / 8, c.what + " y / 8")
    assert is_bf16(c.ref)
    return c


def tail_reference(act, w, bias, activate_padding=None):
    """float64 3 x 3 'same' convolution of the activated NHWC tensor + bias.  activate_padding: the value a kernel that normalised
    and activated its zero padding would hold there, per channel [C] (a planted fault)."""
    a = act.double().permute(0, 3, 1, 2)
    if activate_padding is None:
        a = F.pad(a, (1, 1, 1, 1))
    else:
        a = F.pad(a, (1, 1, 1, 1), value=float("nan"))
        a = torch.where(torch.isnan(a), activate_padding.double().view(1, -1, 1, 1).expand_as(a), a)
    y = F.conv2d(a, w.double().permute(0, 3, 1, 2), bias.double())
    return y.permute(0, 2, 3, 1).contiguous()
