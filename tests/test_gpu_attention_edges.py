"""afldm_attention / afldm_attention_interp (csrc/attn.hip, ONE templated kernel k_attn) at everything attn_check admits and the
FFHQ-shaped tests never launch: every head_dim x dtype x workgroup size x raggedness for both entries, Tq != Tk, query tails,
fp32-only key counts, column-sliced operands, and inputs built so that ONE branch decides the answer (tests/attention_oracle.py):
the -1e30 key mask, the clamped K rows / V^T pieces of a ragged chunk, the tiny path, the first / lazy rescale, interp's restart.
Plus the fused front end (csrc/attnf.hip) with its bounded loop and its row-maxima loop live in one workgroup.

Reference: the fp64 oracle on dtype-rounded inputs.  Tolerances: the project's own for attention (attention_oracle.TOL =
test_gpu_ops.close as test_attention calls it): fp32 max/scale <= 5e-5; bf16 rel-RMS <= 1e-2 and max/scale <= 8e-2.
tests/test_attention_oracle_host.py shows a correct kernel's roundings sit under half of each on every recipe.
Every test prints the error it measured."""
import collections
import math
import os

import pytest
import torch

import attention_oracle as ao

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
HEAD_DIMS = [8, 16, 24, 32]
ENTRIES = ["plain", "interp"]
# (B, Bk, heads, Tq, Tk): the smallest shapes that select each workgroup size through attn_waves (8 waves from Tq >= 256; 2 / 1
# waves need B * heads >= 1024 and Tq <= 64 / <= 32), a ragged and a chunk-aligned key count each.  Tq != Tk nearly everywhere;
# Tq = 264 / 72 / 40 / 24 end in ONE partly filled wave with idle waves behind it (at 8 / 4 / 2 / 1 waves: 8, 8, 8, 24 rows).
W8, W4, W2, W1 = (1, 1, 2), (3, 1, 2), (32, 16, 32), (32, 32, 32)
MATRIX = [("w8-ragged", W8 + (264, 264)), ("w8-even", W8 + (256, 128)), ("w4-ragged", W4 + (72, 200)), ("w4-even", W4 + (40, 64)),
          ("w2-ragged", W2 + (40, 72)), ("w2-even", W2 + (40, 64)), ("w1-ragged", W1 + (24, 136)), ("w1-even", W1 + (24, 64))]
EDGE8, EDGE4 = W8 + (264, 264), W4 + (72, 200)


def _name(dtype):
    return "fp32" if dtype == F32 else "bf16"


def _ops():
    from afldm_amd import ops
    return ops


# ---- inputs and references, built once per (recipe, shape, head_dim, dtype, seed) and shared by the plain and the interp cases
_Case = collections.namedtuple("_Case", "q k v extra")
_cases = collections.OrderedDict()
_refs = collections.OrderedDict()


def _lru(store, key, make, cap):
    if key in store:
        store.move_to_end(key)
    else:
        store[key] = make()
        while len(store) > cap:
            store.popitem(last=False)
    return store[key]


def _case(recipe, shape, d, dtype, seed=0):
    """recipe: ("random",) | ("spiked", keys or None) | ("staircase", step_nats, rising) | ("zero_q",)"""
    B, Bk, heads, Tq, Tk = shape

    def make():
        args = (B, Bk, Tq, Tk, heads, d, dtype)
        if recipe[0] == "random":
            return _Case(*ao.random(*args, seed=seed), None)
        if recipe[0] == "spiked":
            q, k, v, pairs = ao.spiked(*args, seed=seed, keys=recipe[1])
            return _Case(q, k, v, pairs)
        if recipe[0] == "staircase":
            return _Case(*ao.staircase(*args, recipe[1], recipe[2], seed=seed), None)
        assert recipe[0] == "zero_q"
        return _Case(*ao.zero_q(*args, seed=seed), None)
    return (recipe, shape, d, dtype, seed), _lru(_cases, (recipe, shape, d, dtype, seed), make, 8)


def _ref(qc, kc, heads, scale=None):
    """fp64 attention of case qc's queries over case kc's keys / values (qc, kc: (key, case) pairs of _case)"""
    return _lru(_refs, (qc[0], kc[0], scale), lambda: ao.reference(qc[1].q, kc[1].k, kc[1].v, heads, scale), 8)


def _up(x, dtype):
    return x.to(device="cuda", dtype=dtype)


def _alphas(B):
    """distinct per-sample blend weights strictly inside (0, 1)"""
    return torch.tensor([0.37]) if B == 1 else torch.linspace(0.15, 0.85, B)


def _run(entry, src0, src1, shape, dtype, scale=None):
    """launch `entry` on the cases (plain: src0 alone; interp: src0's q over src0 and src1) -> (got on the CPU, fp64 reference)"""
    ops = _ops()
    heads = shape[2]
    c0 = src0[1]
    q, k0, vt0 = _up(c0.q, dtype), _up(c0.k, dtype), _up(ao.vt(c0.v), dtype)
    if entry == "plain":
        return ops.attention(q, k0, vt0, heads, scale=scale).float().cpu(), _ref(src0, src0, heads, scale)
    c1 = src1[1]
    alpha = _alphas(shape[0])
    got = ops.attention_interp(q, k0, vt0, _up(c1.k, dtype), _up(ao.vt(c1.v), dtype), alpha.cuda(), heads, scale=scale)
    a = alpha.double().view(-1, 1, 1)
    return got.float().cpu(), (1 - a) * _ref(src0, src0, heads, scale) + a * _ref(src0, src1, heads, scale)


def _check(group, what, got, ref, dtype):
    bad = int((~torch.isfinite(got)).sum())
    if bad:
        print(f"[attention edges {group}] {what}: {bad} non-finite outputs")
    why, mx, rms = ao.within(got, ref, dtype)
    print(f"[attention edges {group}] {what}: max/scale {mx:.3e} rel-RMS {rms:.3e}")
    assert why is None, f"{what}: {why}"


# ------------------------------------------------------------------------------------------------ a. instantiation matrix
@pytest.mark.parametrize("label,shape,d,dtype,entry",
                         [pytest.param(lb, sh, d, dt, en, id=f"{lb}-d{d}-{_name(dt)}-{en}")
                          for lb, sh in MATRIX for d in HEAD_DIMS for dt in DTYPES for en in ENTRIES])
def test_every_instantiation(label, shape, d, dtype, entry):
    """k_attn<T, ND, NKF, NW, RAGGED, 0, INTERP> for every (head_dim, dtype, waves, raggedness, entry): 128 kernels.  The
    ragged shapes have full chunks in front of the ragged one (key0 > 0 in the clamps, under the two-chunk prefetch)."""
    src0 = _case(("random",), shape, d, dtype, seed=0)
    src1 = _case(("random",), shape, d, dtype, seed=1)
    got, ref = _run(entry, src0, src1, shape, dtype)
    _check("a", f"{label} {shape} d={d} {_name(dtype)} {entry}", got, ref, dtype)


SHORT = [(8, F32), (8, BF16),        # Tk = 8: ONE 16-byte V^T piece per row in bf16, every other piece of the chunk clamped onto it
         (4, F32), (4, BF16),        # Tk = 4: the `tiny` element-wise V^T path in bf16 (a clamped piece would start 4 keys BEFORE the row); one whole piece in fp32
         (68, F32), (100, F32)]      # Tk % 8 == 4 (fp32 only): a live 4-key piece right at the ragged edge, one full chunk in front


@pytest.mark.parametrize("Tk,dtype", SHORT, ids=[f"Tk{t}-{_name(dt)}" for t, dt in SHORT])
@pytest.mark.parametrize("entry", ENTRIES)
def test_short_and_fp32_only_key_counts(entry, Tk, dtype):
    shape = W4 + (72, Tk)
    got, ref = _run(entry, _case(("random",), shape, 24, dtype, 0), _case(("random",), shape, 24, dtype, 1), shape, dtype)
    _check("a", f"Tk={Tk} d=24 {_name(dtype)} {entry}", got, ref, dtype)
    # Tk = 4 / 8 with q = 0: the mean of the 4 / 8 real values; a zero-filled or clamped slot that escaped the mask moves it by >= 1/9
    if Tk <= 8:
        z = _case(("zero_q",), shape, 24, dtype, 0)
        got, ref = _run(entry, z, _case(("random",), shape, 24, dtype, 1), shape, dtype)
        _check("a", f"Tk={Tk} d=24 {_name(dtype)} {entry} zero_q", got, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("entry", ENTRIES)
def test_column_sliced_operands_with_a_ragged_key_count(entry, dtype):
    """q and k are the two halves of a [B, T, 2C] buffer, as linear_split leaves them (leading dimension 2C), T = 200: the K-row
    clamp is computed with ldk - with C instead it lands in another row's q half and live keys of the last chunk are replaced."""
    ops = _ops()
    shape = (3, 3, 2, 200, 200)
    heads, d = 2, 24
    C = heads * d
    src0, src1 = _case(("random",), shape, d, dtype, 0), _case(("random",), shape, d, dtype, 1)
    buf0 = _up(torch.cat([src0[1].q, src0[1].k], dim=2), dtype)
    assert buf0[:, :, C:].stride(1) == 2 * C
    if entry == "plain":
        got = ops.attention(buf0[:, :, :C], buf0[:, :, C:], _up(ao.vt(src0[1].v), dtype), heads)
        ref = _ref(src0, src0, heads)
    else:
        buf1 = _up(torch.cat([src1[1].q, src1[1].k], dim=2), dtype)
        alpha = _alphas(3)
        got = ops.attention_interp(buf0[:, :, :C], buf0[:, :, C:], _up(ao.vt(src0[1].v), dtype), buf1[:, :, C:],
                                   _up(ao.vt(src1[1].v), dtype), alpha.cuda(), heads)
        a = alpha.double().view(-1, 1, 1)
        ref = (1 - a) * _ref(src0, src0, heads) + a * _ref(src0, src1, heads)
    _check("a", f"column slices T=200 {_name(dtype)} {entry}", got.float().cpu(), ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("entry", ENTRIES)
def test_non_default_scale(entry, dtype):
    src0, src1 = _case(("random",), EDGE4, 24, dtype, 0), _case(("random",), EDGE4, 24, dtype, 1)
    got, ref = _run(entry, src0, src1, EDGE4, dtype, scale=0.37)
    _check("a", f"scale=0.37 {_name(dtype)} {entry}", got, ref, dtype)
    assert ao.errors(ref, _ref(src0, src0, 2))[0] > 1e-2          # (the scale reaches the oracle: 0.37 is not 24^-0.5)


# ------------------------------------------------------------------------------------------------ b. numeric edges
PLAIN_RECIPES = [
    # the 30-nat key sits at 0, 63, 64, the first key of the last (ragged) chunk and Tk - 1.  K-ROW CLAMP: fired one row early, or
    # addressed without key0, it replaces the live row Tk - 1 / the last chunk's first row and the spiked query loses its key.
    # V^T-PIECE CLAMP: fired one piece early the spiked row returns the wrong 4 / 8 keys' values.  FIRST RESCALE: a spike in
    # chunk 0 makes the first reference 43 log2 units; LAZY RESCALE: spikes at 64 / the last chunk move it by 43 in ONE step
    ("spiked", None),
    # LAZY RESCALE in every chunk (17 log2 units each, four in a row at Tk = 264, the last one inside the ragged chunk, each
    # exactly at a 64-key boundary); in bf16 the reference is rounded to bf16 and rides in Q: without the rescale P overflows
    # bf16's 8 bits of mantissa at 2^69, with a wrong delta numerator and denominator disagree
    ("staircase", 12.0, True),
    # FIRST RESCALE takes the largest reference at once; every later chunk underflows to P = 0 - the -1e30 mask then meets
    # s - m of -69: a mask applied as an offset instead of a value would not matter here, the ragged mean below catches it
    ("staircase", 12.0, False),
    # 7 log2 units per chunk: P = 2^7 in the chunk after a reference move, then a move (14 > 10): P > 1 in bf16, unrescaled
    ("staircase", 5.0, True),
    # THE -1e30 MASK: q = 0 gives the plain mean over the Tk real keys; ONE unmasked clamped key (a copy of key Tk - 1) or one
    # masked real key moves every output by ~1/Tk of a V entry: 5e-3 of scale against 5e-5 in fp32
    ("zero_q",),
]
EDGE_CASES = [pytest.param(sh, d, dt, id=f"{lb}-d{d}-{_name(dt)}")
              for lb, sh in (("w8", EDGE8), ("w4", EDGE4)) for d in (8, 24, 32) for dt in DTYPES]


@pytest.mark.parametrize("recipe", PLAIN_RECIPES, ids=lambda r: "-".join(str(x) for x in r if x is not None))
@pytest.mark.parametrize("shape,d,dtype", EDGE_CASES)
def test_numeric_edges_plain(shape, d, dtype, recipe):
    src = _case(recipe, shape, d, dtype)
    got, ref = _run("plain", src, None, shape, dtype)
    what = f"{recipe} {shape} d={d} {_name(dtype)}"
    _check("b", what, got, ref, dtype)
    if recipe[0] == "spiked":       # the spiked rows alone, per row: v of their key (the whole-tensor figures average them away)
        B, Bk, heads, Tq, Tk = shape
        for i, j in src[1].extra:
            _check("b", f"{what} row {i} -> key {j}", got[:, i], ref[:, i], dtype)
            assert (ref[:, i] - src[1].v[:, j].double().repeat_interleave(B // Bk, 0)).abs().max() <= 1e-5


INTERP_ARRANGEMENTS = [
    # THE RESTART "exactly as at chunk 0": source 1's first key scores 43 log2 units against a reference that must be 0 again,
    # and its last key sits in source 1's ragged chunk: a reference, denominator or -m_run channel kept from source 0 shows at once
    ("spike-in-source-1", ("random",), ("spiked", (0, -1))),
    # source 0 ends with the reference at 69 log2 units, in its ragged tail, while source 1's first chunks are already prefetched:
    # WITHOUT THE RESTART source 1's ordinary scores are 2^-69 -> its row sums vanish and alpha * O1 / l1 is 0 / 0
    ("staircase-then-random", ("staircase", 12.0, True), ("random",)),
    # ... and the lazy rescale after the boundary: source 1 climbs 17 log2 units per chunk from a fresh reference
    ("random-then-staircase", ("random",), ("staircase", 12.0, True)),
]


@pytest.mark.parametrize("label,r0,r1", INTERP_ARRANGEMENTS, ids=[a[0] for a in INTERP_ARRANGEMENTS])
@pytest.mark.parametrize("shape,d,dtype", EDGE_CASES)
def test_numeric_edges_interp(shape, d, dtype, label, r0, r1):
    """q always comes from the structured source (the spike / the staircase channel is a property of q AND k)."""
    Tk = shape[4]
    fix = lambda r: ("spiked", (0, Tk - 1)) if r[0] == "spiked" else r
    c0, c1 = _case(fix(r0), shape, d, dtype, seed=0), _case(fix(r1), shape, d, dtype, seed=1)
    qsrc = c1 if r0 == ("random",) else c0
    ops = _ops()
    heads = shape[2]
    alpha = _alphas(shape[0])
    got = ops.attention_interp(_up(qsrc[1].q, dtype), _up(c0[1].k, dtype), _up(ao.vt(c0[1].v), dtype), _up(c1[1].k, dtype),
                               _up(ao.vt(c1[1].v), dtype), alpha.cuda(), heads).float().cpu()
    a = alpha.double().view(-1, 1, 1)
    ref = (1 - a) * _ref(qsrc, c0, heads) + a * _ref(qsrc, c1, heads)
    _check("b", f"interp {label} {shape} d={d} {_name(dtype)}", got, ref, dtype)


# ------------------------------------------------------------------------------------------------ c. canaries
CANARY = [(W4 + (72, 200), 24), (W2 + (40, 72), 8),
          (W4 + (72, 4), 24)]     # THE TINY PATH (bf16): a 16-byte read of a 4-key V^T row runs into the next row and, at the last row, into the guard


@pytest.mark.parametrize("shape,d", CANARY, ids=[f"{s[0]}x{s[2]}-Tq{s[3]}-Tk{s[4]}-d{d}" for s, d in CANARY])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("entry", ENTRIES)
def test_masked_slots_never_hold_data_from_beside_the_operands(entry, dtype, shape, d):
    """Every operand is surrounded by NaN inside its own allocation: q / k rows carry 8 NaN columns behind their head channels
    (leading dimension C + 8), vt and out sit 64 elements inside NaN-filled buffers.  Masked slots multiply by P = 0, but
    0 x NaN = NaN: a K row, Q fragment or V^T PIECE (the last channel row's pieces past Tk are the ones whose unclamped address
    leaves the operand) taken from beside the operand poisons the P V product, which random finite neighbours would hide.  All
    reads and writes stay inside the torch allocations; the guards around `out` must still be NaN afterwards."""
    ops = _ops()
    B, Bk, heads, Tq, Tk = shape
    C = heads * d
    src0, src1 = _case(("random",), shape, d, dtype, 0), _case(("random",), shape, d, dtype, 1)

    def place(c):
        kv, _ = ao.canary_wide(c.k, dtype, "cuda")
        vv, vwhole = ao.canary((Bk, C, Tk), dtype, 64, "cuda")
        vv.copy_(_up(ao.vt(c.v), dtype))
        assert ao.guards_intact(vwhole, (Bk, C, Tk)) and kv.stride(1) == C + 8
        return kv, vv
    qv, _ = ao.canary_wide(src0[1].q, dtype, "cuda")
    out, owhole = ao.canary((B, Tq, C), dtype, 64, "cuda")
    k0, vt0 = place(src0[1])
    if entry == "plain":
        res = ops.attention(qv, k0, vt0, heads, out=out)
        ref = _ref(src0, src0, heads)
    else:
        k1, vt1 = place(src1[1])
        alpha = _alphas(B)
        res = ops.attention_interp(qv, k0, vt0, k1, vt1, alpha.cuda(), heads, out=out)
        a = alpha.double().view(-1, 1, 1)
        ref = (1 - a) * _ref(src0, src0, heads) + a * _ref(src0, src1, heads)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    _check("c", f"canary {shape} d={d} {_name(dtype)} {entry}", out.float().cpu(), ref, dtype)
    assert ao.guards_intact(owhole, (B, Tq, C)), "the kernel wrote outside its output"


# ------------------------------------------------------------------------------------------------ d. alpha in {0, 1}
@pytest.mark.parametrize("d", HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_interp_with_alpha_0_or_1_is_the_single_source_launch(dtype, d):
    """attn.hip's header: at the boundary the running max / row sums restart exactly as at chunk 0, so source 1 alone is the same
    arithmetic as a single-source launch on it; source 0's O is normalised by (1 - alpha) / l = 1 / l.  Bit for bit, at the ragged
    4-wave shape (source 0's ragged tail, then source 1's chunks from the prefetch registers)."""
    ops = _ops()
    shape = EDGE4
    B, heads = shape[0], shape[2]
    c0, c1 = _case(("random",), shape, d, dtype, 0)[1], _case(("random",), shape, d, dtype, 1)[1]
    q, k0, vt0, k1, vt1 = (_up(x, dtype) for x in (c0.q, c0.k, ao.vt(c0.v), c1.k, ao.vt(c1.v)))
    for a, (k, v) in ((0.0, (k0, vt0)), (1.0, (k1, vt1))):
        got = ops.attention_interp(q, k0, vt0, k1, vt1, torch.full((B,), a, device="cuda"), heads)
        one = ops.attention(q, k, v, heads)
        diff = float((got.float() - one.float()).abs().max())
        print(f"[attention edges d] alpha={a} d={d} {_name(dtype)}: max |interp - single source| = {diff:.3e}")
        assert torch.equal(got, one), (a, diff)


# ------------------------------------------------------------------------------------------------ e. fused front end, both loops live
def _hot_token_block(T, C, heads, B=2, G=32, eps=1e-5, hot=5):
    """Ordinary tokens, except token `hot` of every sample = 60 sqrt(C) u for a unit vector u: after GroupNorm that token is
    ~sqrt(T) in every channel.  to_k loses u AND the normalised hot rows themselves (GroupNorm's per-channel scale turns u a
    little, so u alone leaves the hot key ten times an ordinary one), projected out before rounding to bf16; to_q gains a
    rank-one term along the normalised hot row (a unit vector per head, times 2): the hot token's QUERY is huge, its key is
    not, and the other tokens' queries change by O(1)."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(T + C + 1)
    x = torch.randn(B, T, C, generator=gen) * (1.0 + torch.rand(1, 1, C, generator=gen)) + 0.5 * torch.randn(1, 1, C, generator=gen)
    gamma, beta = 0.5 + torch.rand(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
    ws = [torch.randn(C, C, generator=gen) / C ** 0.5 for _ in range(3)]
    bs = [0.2 * torch.randn(C, generator=gen) for _ in range(3)]
    u = torch.randn(C, generator=gen)
    u = u / u.norm()
    r = torch.randn(C, generator=gen).view(heads, C // heads)
    x[:, hot] = 60.0 * math.sqrt(C) * u
    xb = x.to(BF16)
    hn = F.group_norm(xb.float().transpose(1, 2), G, gamma, beta, eps).transpose(1, 2)[:, hot]          # [B, C]
    basis, _ = torch.linalg.qr(torch.cat([u[None], hn], 0).double().T)                                 # [C, 1 + B], orthonormal
    wk = ws[1].double()
    ws[1] = (wk - (wk @ basis) @ basis.T).float()
    assert (ws[1] @ u).abs().max() <= 1e-5
    hd = hn.mean(0) / hn.mean(0).norm()
    ws[0] = ws[0] + 2.0 * torch.outer((r / r.norm(dim=1, keepdim=True)).reshape(C), hd)
    return xb, gamma, beta, [w.to(BF16) for w in ws], bs


def _bounded_loop_gaps(xb, gamma, beta, wb, bs, heads, G=32, eps=1e-5, h=None):
    """The kernel's own predicate from the bf16-rounded projections, per 32-query tile: max over the tile's queries of
    sqrt(|q|^2 max|k|^2) * 1.002 + 0.01 - m_run, q in log2 units (scale * log2 e folded in), m_run = the row maximum over the
    first 32 keys, rounded to bf16.  A wave takes the bounded loop when this is <= 80 for all of its queries.  [B, heads, T / 32]
    h: the normalised tokens [B, T, C], where the caller dictates the statistics instead of taking them from the data."""
    import torch.nn.functional as F
    B, T, C = xb.shape
    d = C // heads
    if h is None:
        h = F.group_norm(xb.float().transpose(1, 2), G, gamma, beta, eps).transpose(1, 2)
    q = ao.rnd(F.linear(h, wb[0].float(), bs[0]) * (d ** -0.5 * ao.LOG2E), BF16).view(B, T, heads, d).transpose(1, 2)
    k = ao.rnd(F.linear(h, wb[1].float(), bs[1]), BF16).view(B, T, heads, d).transpose(1, 2)
    kmax2 = k.pow(2).sum(-1).max(-1).values
    m_run = ao.rnd((q @ k[:, :, :32].transpose(2, 3)).max(-1).values, BF16)
    gap = (q.pow(2).sum(-1) * kmax2[..., None]).sqrt() * 1.002 + 0.01 - m_run
    return gap.view(B, heads, T // 32, 32).max(-1).values


@pytest.mark.parametrize("T,C,heads", [(256, 64, 4), (256, 384, 16)])
def test_attn_block_fused_with_both_loops_live_in_one_workgroup(T, C, heads):
    """k_attn_fused chooses per WAVE (__all(safe)) between the bounded loop and the row-maxima loop; neither fast_step nor step
    holds a workgroup barrier (K / V^T are resident in LDS), so one workgroup may run both.  One hot token per sample (in the
    first 32-query tile) sends its wave to the row-maxima loop while every other wave keeps the bounded one."""
    from test_gpu_r04 import _attn_block_reference
    ops = _ops()
    B, G, eps, hot = 2, 32, 1e-5, 5
    xb, gamma, beta, wb, bs = _hot_token_block(T, C, heads, B, G, eps, hot)
    gaps = _bounded_loop_gaps(xb, gamma, beta, wb, bs, heads, G, eps)
    hot_gap, rest_gap = gaps[:, :, hot // 32], torch.cat([gaps[:, :, :hot // 32], gaps[:, :, hot // 32 + 1:]], -1)
    print(f"[attention edges e] T={T} C={C}: predicate bound - m_run (limit 80): hot tile {float(hot_gap.min()):.1f} .. "
          f"{float(hot_gap.max()):.1f}, other tiles <= {float(rest_gap.max()):.1f}")
    assert hot_gap.min() >= 80 + 20 and rest_gap.max() <= 80 - 20
    ref = _attn_block_reference(xb.float(), gamma, beta, G, eps, *[w.float() for w in wb], *bs, heads)
    xg, gg, bg = xb.cuda(), gamma.cuda(), beta.cuda()
    side = int(T ** 0.5)
    scale = (C // heads) ** -0.5
    stats = ops.gn_stats(xg.view(B, side, side, C), G)
    wpack = ops.pack_weight(torch.cat(wb, 0).float().cuda(), BF16)
    bpack = torch.cat(bs, 0).cuda()
    got = ops.attn_block_fused(xg, stats, gg, bg, G, eps, wpack, bpack, heads, scale)
    hn = ops.gn_apply(xg.view(B, side, side, C), stats, gg, bg, G, eps, act=0).view(B, T, C)
    qk, vt = ops.linear_split(hn, wpack, bpack, 2 * C)
    old = ops.attention(qk[:, :, :C], qk[:, :, C:], vt, heads, scale=scale)
    os.environ["AFLDM_ATTNF_SLOW"] = "1"
    try:
        slow = ops.attn_block_fused(xg, stats, gg, bg, G, eps, wpack, bpack, heads, scale)
    finally:
        del os.environ["AFLDM_ATTNF_SLOW"]
    torch.cuda.synchronize()
    got, old, slow = got.float().cpu(), old.float().cpu(), slow.float().cpu()
    rest = torch.ones(T, dtype=torch.bool)
    rest[hot // 32 * 32:hot // 32 * 32 + 32] = False
    figs = dict(ref=ao.errors(got, ref)[1], three_launch=ao.errors(got, old)[1], slow_ref=ao.errors(slow, ref)[1],
                slow_rest=ao.errors(slow[:, rest], got[:, rest])[1])
    print(f"[attention edges e] T={T} C={C}: rel-RMS vs fp32 reference {figs['ref']:.3e}, vs three-launch path {figs['three_launch']:.3e}; "
          f"row-maxima loop forced: vs reference {figs['slow_ref']:.3e}, vs default outside the hot tile {figs['slow_rest']:.3e}")
    assert max(figs.values()) <= 2e-2, figs
    # the hot tile's wave takes the row-maxima loop in both runs: the same instructions on the same data
    assert torch.equal(slow[:, ~rest], got[:, ~rest])


# ------------------------------------------------------------------------------------------------ f. refusals
def test_attention_refuses_what_attn_check_excludes_and_stays_usable():
    from afldm_amd._lib import AfldmError
    ops = _ops()

    def operands(dtype, B=3, Bk=1, heads=2, Tq=16, Tk=16, d=24):
        C = heads * d
        z = lambda *s: torch.zeros(*s, device="cuda", dtype=dtype)
        return [z(B, Tq, C), z(Bk, Tk, C), z(Bk, C, Tk), heads]

    def wide_q(extra):                  # leading dimension C + extra
        a = operands(BF16)
        a[0] = torch.zeros(3, 16, 48 + extra, device="cuda", dtype=BF16)[:, :, :48]
        return a

    def shifted_q():                    # starts 4 bf16 elements (8 bytes) into its buffer
        a = operands(BF16)
        a[0] = torch.zeros(3 * 16 * 48 + 8, device="cuda", dtype=BF16)[4:4 + 3 * 16 * 48].view(3, 16, 48)
        return a
    assert wide_q(8)[0].stride(1) == 56 and shifted_q()[0].data_ptr() % 16 == 8
    refused = [("bf16 Tk=12", operands(BF16, Tk=12), "Tk"), ("fp32 Tk=6", operands(F32, Tk=6), "Tk"),
               ("d=12", operands(BF16, d=12), "head_dim"), ("d=40", operands(F32, d=40), "head_dim"),
               ("B % Bk", operands(BF16, B=3, Bk=2), "bad shape"), ("ldq = C + 4", wide_q(4), "leading dims"),
               ("q + 4 elements", shifted_q(), "aligned")]
    shape, dtype = EDGE4, BF16
    src = _case(("random",), shape, 24, dtype, 0)
    for what, args, match in refused:
        with pytest.raises(AfldmError, match=match):
            ops.attention(*args)
        got, ref = _run("plain", src, None, shape, dtype)          # the library is still usable, and right
        _check("f", f"valid call after refusing {what}", got, ref, dtype)
    ops.attention(*wide_q(8))                                       # (the same placements are accepted once legal)
