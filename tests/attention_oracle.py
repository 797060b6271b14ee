"""CPU oracle of softmax attention (afldm_attention / afldm_attention_interp), the seeded input recipes of the edge tests,
the NaN-guarded operand placements, and a CPU model of the kernel's roundings.

Layouts: q [B, Tq, C], k / v [Bk, Tk, C] token-major, C = heads * d, Bk | B; query sample b reads key sample
b // (B // Bk), as the kernel does.  (The kernel takes V channel-major: vt(v) below.)

Every recipe returns fp32 tensors that were ROUNDED THROUGH the test dtype, so the oracle and the kernel see identical
numbers; the oracle itself is float64 and written out plainly: matmul, softmax, matmul.

Tolerances (TOL) are the project's own for attention, test_gpu_ops.py::close as test_attention calls it:
fp32 max|got - ref| <= 5e-5 max|ref|; bf16 rel-RMS <= 1e-2 and max|got - ref| <= 8e-2 max|ref|."""
import math

import torch

LOG2E = 1.4426950408889634
KC = 64                 # keys per staged chunk of k_attn
LAZY_TAU = 10.0         # the kernel moves its reference when a row maximum outgrows it by 2^10
SPIKE_NATS = 30.0
TOL = {torch.float32: dict(max=5e-5), torch.bfloat16: dict(rms=1e-2, max=8e-2)}


def rnd(x, dtype):
    return x.to(dtype).to(torch.float32)


def vt(v):
    """[Bk, Tk, C] -> the kernel's channel-major [Bk, C, Tk]"""
    return v.transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ the oracle
def _heads(x, heads):
    B, T, C = x.shape
    return x.double().view(B, T, heads, C // heads).transpose(1, 2)          # [B, heads, T, d]


def scores(q, k, heads, scale=None):
    """fp64 q k^T * scale in nats, [B, heads, Tq, Tk]"""
    B, Bk = q.shape[0], k.shape[0]
    assert B % Bk == 0
    d = q.shape[2] // heads
    scale = d ** -0.5 if scale is None else scale
    kb = torch.arange(B) // (B // Bk)
    return _heads(q, heads) @ _heads(k, heads)[kb].transpose(2, 3) * scale


def reference(q, k, v, heads, scale=None):
    B, Tq, C = q.shape
    kb = torch.arange(B) // (B // k.shape[0])
    p = torch.softmax(scores(q, k, heads, scale), dim=-1)
    return (p @ _heads(v, heads)[kb]).transpose(1, 2).reshape(B, Tq, C)


def reference_interp(q, k0, v0, k1, v1, alpha, heads, scale=None):
    a = torch.as_tensor(alpha).double().view(-1, 1, 1)
    return (1 - a) * reference(q, k0, v0, heads, scale) + a * reference(q, k1, v1, heads, scale)


def errors(got, ref):
    """(max|got - ref| / max|ref|, rel-RMS) in float64"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    diff = got - ref
    return (float(diff.abs().max() / ref.abs().max().clamp_min(1e-30)),
            float(diff.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30)))


def within(got, ref, dtype, frac=1.0):
    """None when got meets frac x TOL[dtype] against ref, else the reason; also returns the two error figures"""
    mx, rms = errors(got, ref)
    t = TOL[dtype]
    why = None
    if mx > frac * t["max"]:
        why = f"max/scale {mx:.3e} > {frac * t['max']:.1e}"
    elif "rms" in t and rms > frac * t["rms"]:
        why = f"rel-RMS {rms:.3e} > {frac * t['rms']:.1e}"
    return why, mx, rms


# ------------------------------------------------------------------------------------------------ input recipes
def _base(B, Bk, Tq, Tk, heads, d, seed):
    """N(0, 1) with asymmetric per-channel scales in [0.5, 1.5) (different for q, k and v) and a small per-channel offset
    on v: no two channels, heads, keys or samples are exchangeable, so a transposed or permuted fragment cannot pass."""
    g = torch.Generator().manual_seed(1000 + seed)
    C = heads * d
    out = []
    for n, t in ((B, Tq), (Bk, Tk), (Bk, Tk)):
        out.append(torch.randn(n, t, C, generator=g) * (0.5 + torch.rand(1, 1, C, generator=g)))
    out[2] = out[2] + 0.25 * torch.randn(1, 1, C, generator=g)
    return out


def random(B, Bk, Tq, Tk, heads, d, dtype, seed=0):
    return tuple(rnd(x, dtype) for x in _base(B, Bk, Tq, Tk, heads, d, seed))


def spike_keys(Tk):
    """the key positions that exist for Tk out of {0, 63, 64, Tk - 1, the first key of the last chunk}"""
    last0 = (Tk - 1) // KC * KC
    return sorted({j for j in (0, 63, 64, Tk - 1, last0) if 0 <= j < Tk})


def spike_rows(Tq, n):
    """n distinct query rows: the first wave, a second 16-query fragment, the last row (the partly filled wave) ..."""
    rows = []
    for i in (5, Tq - 1, 16 % Tq, Tq // 2, 37 % Tq, 1, 2, 3):
        if i not in rows and len(rows) < n:
            rows.append(i)
    assert len(rows) == n, (Tq, n)
    return rows


def spiked(B, Bk, Tq, Tk, heads, d, dtype, seed=0, keys=None):
    """random, with pairs (query i, key j): k_h[j] = q_h[i] * 30 sqrt(d) / |q_h[i]|^2 for every head, so that the pair's score
    is 30 nats (43 log2 units) at every head_dim with the default scale.  The spiked query rows of one head are made
    orthogonal (Gram-Schmidt, at most 5 <= d of them) with norm sqrt(d), and equal across the query samples that share a
    key sample: the other spiked keys then score 0 against them and the random keys score N(0, < 1.5^2), which is what keeps
    20 nats of margin at d = 8.  Returns q, k, v, pairs."""
    q, k, v = _base(B, Bk, Tq, Tk, heads, d, seed)
    keys = spike_keys(Tk) if keys is None else list(keys)
    rows = spike_rows(Tq, len(keys))
    assert len(keys) <= d
    rep = B // Bk
    for kb in range(Bk):
        qs = q[kb * rep, rows].view(len(rows), heads, d).double()
        for n in range(len(rows)):                          # Gram-Schmidt per head
            for m in range(n):
                qs[n] -= (qs[n] * qs[m]).sum(-1, keepdim=True) / d * qs[m]
            qs[n] *= math.sqrt(d) / qs[n].norm(dim=-1, keepdim=True)
        for b in range(kb * rep, (kb + 1) * rep):
            q[b, rows] = qs.reshape(len(rows), heads * d).float()
        k[kb, keys] = (qs * (SPIKE_NATS * math.sqrt(d) / d)).reshape(len(keys), heads * d).float()    # |q_h|^2 = d
    return rnd(q, dtype), rnd(k, dtype), rnd(v, dtype), list(zip(rows, keys))


def staircase(B, Bk, Tq, Tk, heads, d, dtype, step_nats, rising, seed=0):
    """random (q and k halved), plus one shared channel per head: q[..., h d] = 4, k[j, h d] = level(j) step sqrt(d) / 4 with
    level = j // 64 (reversed when falling): every 64-key chunk lifts (drops) ALL scores of the head by `step` nats.
    step = 12 (17 log2 units > LAZY_TAU): the reference moves in every chunk when rising.  step = 5 (7 log2 units): no
    chunk outgrows its predecessor by 2^10, so P reaches ~2^7 (and, two levels above the reference, 2^10) unrescaled."""
    q, k, v = _base(B, Bk, Tq, Tk, heads, d, seed)
    level = torch.arange(Tk) // KC
    if not rising:
        level = (Tk - 1) // KC - level
    q, k = 0.5 * q, 0.5 * k          # the random part of a score: std ~0.3 nats, so a chunk maximum moves by step +- 1.5 nats
    q[:, :, ::d] = 4.0
    k[:, :, ::d] = (level.float() * (step_nats * math.sqrt(d) / 4.0)).view(1, Tk, 1)
    return rnd(q, dtype), rnd(k, dtype), rnd(v, dtype)


def zero_q(B, Bk, Tq, Tk, heads, d, dtype, seed=0):
    """q = 0: every score is 0 and the answer is the plain mean of V over the Tk real keys; one wrongly masked or unmasked
    key moves it by 1 / Tk of a V entry."""
    q, k, v = _base(B, Bk, Tq, Tk, heads, d, seed)
    return torch.zeros_like(q), rnd(k, dtype), rnd(v, dtype)


def chunk_row_maxima(q, k, heads, scale=None):
    """[B, heads, Tq, nchunks]: the row maximum of every 64-key chunk, in log2 units"""
    s = scores(q, k, heads, scale) * LOG2E
    return torch.stack([c.max(-1).values for c in s.split(KC, dim=-1)], dim=-1)


# ------------------------------------------------------------------------------------------------ NaN-guarded placements
def canary(shape, dtype, pad=64, device="cpu"):
    """(view, whole): `whole` is ONE flat NaN-filled allocation, `view` a contiguous tensor of `shape` inside it, `pad`
    elements from either end (pad a multiple of 64: the view stays 16-byte aligned).  Nothing outside `whole` is touched."""
    assert pad > 0 and pad % 64 == 0
    n = math.prod(shape)
    whole = torch.full((n + 2 * pad,), float("nan"), dtype=dtype, device=device)
    return whole[pad:pad + n].view(shape), whole


def guards_intact(whole, shape, pad=64):
    n = math.prod(shape)
    return bool(torch.isnan(whole[:pad]).all() and torch.isnan(whole[pad + n:]).all())


def canary_wide(x, dtype, device="cpu"):
    """(view, whole) for token-major q / k [B, T, C]: whole is [B, T, C + 8] with x in its first C columns and NaN in the
    last 8, view = whole[:, :, :C] (leading dimension C + 8): a read past a row's head channels meets NaN."""
    B, T, C = x.shape
    whole = torch.full((B, T, C + 8), float("nan"), dtype=dtype, device=device)
    whole[:, :, :C] = x.to(device=device, dtype=dtype)
    return whole[:, :, :C], whole


# ------------------------------------------------------------------------------------------------ model of the roundings
def kernel_model(q, k, v, heads, dtype, scale=None):
    """What a CORRECT k_attn computes, rounding for rounding (not its instruction order): Q * scale * log2(e) rounded to the
    dtype; scores in fp32; per 64-key chunk the lazy reference (rounded to the dtype, moved for a whole 32-query wave when
    any of its row maxima outgrows it by 2^10; set to the row maximum at chunk 0); P = 2^(s - m) rounded to the dtype;
    numerator and denominator accumulated in fp32 from the rounded P; one rounding of the quotient.  fp32 [B, Tq, C]."""
    B, Tq, C = q.shape
    Bk, Tk, _ = k.shape
    d = C // heads
    scale = d ** -0.5 if scale is None else scale
    f32 = torch.float32
    sl2 = torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    kb = torch.arange(B) // (B // Bk)
    qh = rnd(q.to(f32) * sl2, dtype).view(B, Tq, heads, d).transpose(1, 2)
    kh = k.to(f32).view(Bk, Tk, heads, d).transpose(1, 2)[kb]
    vh = v.to(f32).view(Bk, Tk, heads, d).transpose(1, 2)[kb]
    s_all = qh @ kh.transpose(2, 3)                                        # fp32 [B, heads, Tq, Tk]
    m_run = torch.zeros(B, heads, Tq, dtype=f32)
    o = torch.zeros(B, heads, Tq, d, dtype=f32)
    l = torch.zeros(B, heads, Tq, dtype=f32)
    wave = torch.arange(Tq) // 32
    for c, key0 in enumerate(range(0, Tk, KC)):
        s = s_all[..., key0:key0 + KC] - m_run[..., None]
        mloc = s.max(-1).values
        if c == 0:
            move = torch.ones_like(mloc, dtype=torch.bool)
            m_new = rnd(m_run + mloc, dtype)
        else:
            hot = torch.stack([(mloc[..., wave == w] > LAZY_TAU).any(-1) for w in range(int(wave.max()) + 1)], -1)
            move = hot[..., wave]
            m_new = rnd(m_run + mloc.clamp_min(0.0), dtype)
        m_new = torch.where(move, m_new, m_run)
        delta = m_new - m_run
        m_run = m_new
        alpha = torch.exp2(-delta)
        p = rnd(torch.exp2(s - delta[..., None]), dtype)
        o = o * alpha[..., None] + p @ vh[:, :, key0:key0 + KC]
        l = l * alpha + p.sum(-1)
    return rnd((o / l[..., None]).transpose(1, 2).reshape(B, Tq, C), dtype)
