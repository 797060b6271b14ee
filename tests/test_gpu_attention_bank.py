"""afldm_attention_bank (csrc/attn.hip, k_attn<..., INTERP = true, BANK = true>): every sample of the batch names its own two
sources in a bank of S stored K / V^T pairs and its own blend weight, both read from device memory when the kernel runs.

Shapes: the smallest of test_gpu_attention_edges.py's matrix that select each workgroup size and raggedness (8 waves from
Tq >= 256, 4 waves above 64 queries, 2 / 1 waves need B * heads >= 1024 and Tq <= 64 / <= 32); the bank replaces the matrix's
Bk, and the 8- / 4-wave shapes - whose wave count does not depend on the batch - run at B = 4 so that one launch holds every kind
of source row.  Reference: the fp64 oracle (tests/attention_oracle.py) per sample and source on dtype-rounded inputs, within the
project's own bound for this kernel family (attention_oracle.TOL).  Every test prints the error it measured."""
import collections

import pytest
import torch

import attention_oracle as ao

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
# label -> (B, heads, Tq, Tk)
SHAPES = collections.OrderedDict([("w8-ragged", (4, 2, 264, 264)), ("w4-ragged", (4, 2, 72, 200)), ("w2-even", (32, 32, 40, 64)),
                                  ("w1-ragged", (32, 32, 24, 136))])
# beyond the matrix: a chunk-aligned key count of THREE chunks - with alpha 0 the stream has an odd number of steps and ends in
# the middle of a step pair, and the loads past its end reload the last chunk (the chunk-aligned loader)
EXTRA = collections.OrderedDict([("w4-even-3-chunks", (4, 2, 72, 192))])
SHAPES.update(EXTRA)
CASES = [pytest.param(lb, d, dt, id=f"{lb}-d{d}-{'fp32' if dt == F32 else 'bf16'}")
         for lb in SHAPES if lb not in EXTRA for d in ((8, 16, 24, 32) if lb == "w4-ragged" else (8, 32)) for dt in DTYPES]
FEW = [pytest.param(lb, d, dt, id=f"{lb}-d{d}-{'fp32' if dt == F32 else 'bf16'}")
       for lb, d in (("w8-ragged", 8), ("w4-ragged", 24), ("w2-even", 32), ("w1-ragged", 8), ("w4-even-3-chunks", 24)) for dt in DTYPES]


def _name(dtype):
    return "fp32" if dtype == F32 else "bf16"


def _ops():
    from afldm_amd import ops
    return ops


def _up(x, dtype):
    return x.to(device="cuda", dtype=dtype)


_inputs = collections.OrderedDict()


def _case(label, d, dtype, S):
    """(q [B], k [S], v [S]) dtype-rounded fp32 on the CPU, and refs[s] = the fp64 attention of every query sample over bank
    slot s: built once per (shape, head_dim, dtype, S) and shared by the tests, never written."""
    key = (label, d, dtype, S)
    if key not in _inputs:
        B, heads, Tq, Tk = SHAPES[label]
        q, k, v = ao.random(B, S, Tq, Tk, heads, d, dtype, seed=7 + S)
        refs = [ao.reference(q, k[s:s + 1], v[s:s + 1], heads) for s in range(S)]
        _inputs[key] = (q, k, v, refs)
        while len(_inputs) > 6:
            _inputs.popitem(last=False)
    return _inputs[key]


def _table(B, rows):
    """rows = [(s0, s1, alpha)] repeated over the batch -> (src int32 [B, 2], alpha fp32 [B]) on the device, and the host rows"""
    host = [rows[b % len(rows)] for b in range(B)]
    src = torch.tensor([[r[0], r[1]] for r in host], dtype=torch.int32, device="cuda")
    alpha = torch.tensor([r[2] for r in host], dtype=torch.float32, device="cuda")
    return src, alpha, host


def _blend(refs, host):
    return torch.stack([(1 - a) * refs[s0][b] + a * refs[s1][b] for b, (s0, s1, a) in enumerate(host)])


def _check(what, got, ref, dtype):
    why, mx, rms = ao.within(got, ref, dtype)
    print(f"[attention bank] {what}: max/scale {mx:.3e} rel-RMS {rms:.3e}")
    assert why is None, f"{what}: {why}"


# (0, 1), (2, 0), (1, 1) blended with weights strictly inside (0, 1); (s, other) with alpha exactly 0: the skip
ROWS = [(0, 1, 0.37), (2, 0, 0.81), (1, 1, 0.15), (2, 1, 0.0), (0, 2, 0.0)]


# ------------------------------------------------------------------------------------------------ a. against the fp64 oracle
@pytest.mark.parametrize("label,d,dtype", CASES)
def test_bank_against_the_fp64_oracle(label, d, dtype):
    ops = _ops()
    B, heads, Tq, Tk = SHAPES[label]
    q, k, v, refs = _case(label, d, dtype, 3)
    src, alpha, host = _table(B, ROWS)
    assert {r[:2] for r in host} >= {(0, 1), (2, 0), (1, 1)} and any(r[2] == 0.0 and r[0] != r[1] for r in host)
    got = ops.attention_bank(_up(q, dtype), _up(k, dtype), _up(ao.vt(v), dtype), src, alpha, heads)
    assert got.shape == (B, Tq, heads * d) and got.dtype == dtype
    _check(f"{label} d={d} {_name(dtype)}", got.float().cpu(), _blend(refs, host), dtype)


# ------------------------------------------------------------------------------------------------ b. bit for bit at the same B
@pytest.mark.parametrize("label,d,dtype", CASES + [c for c in FEW if c.values[0] in EXTRA])
def test_bank_is_the_interp_launch_bit_for_bit(label, d, dtype):
    """S = 2 with every row (0, 1) is afldm_attention_interp on the two slots; in a mixed table row b is row b of the interp launch
    at the same B (the same workgroup size) over bank[src[b, 0]] and bank[src[b, 1]]; rows with alpha 0 are ops.attention."""
    ops = _ops()
    B, heads, Tq, Tk = SHAPES[label]
    q, k, v, _ = _case(label, d, dtype, 2)
    qd, kd, vd = _up(q, dtype), _up(k, dtype), _up(ao.vt(v), dtype)
    alpha = torch.linspace(0.15, 0.85, B, device="cuda")
    src = torch.tensor([[0, 1]] * B, dtype=torch.int32, device="cuda")
    got = ops.attention_bank(qd, kd, vd, src, alpha, heads)
    want = ops.attention_interp(qd, kd[0:1], vd[0:1], kd[1:2], vd[1:2], alpha, heads)
    print(f"[attention bank] {label} d={d} {_name(dtype)} S=2 all (0, 1): max |bank - interp| = "
          f"{float((got.float() - want.float()).abs().max()):.3e}")
    assert torch.equal(got, want)
    q, k, v, _ = _case(label, d, dtype, 3)
    qd, kd, vd = _up(q, dtype), _up(k, dtype), _up(ao.vt(v), dtype)
    src, alpha, host = _table(B, ROWS)
    got = ops.attention_bank(qd, kd, vd, src, alpha, heads)
    for s0, s1 in sorted({r[:2] for r in host}):
        want = ops.attention_interp(qd, kd[s0:s0 + 1], vd[s0:s0 + 1], kd[s1:s1 + 1], vd[s1:s1 + 1], alpha, heads)
        one = ops.attention(qd, kd[s0:s0 + 1], vd[s0:s0 + 1], heads)
        for b, r in enumerate(host):
            if r[:2] == (s0, s1):
                assert torch.equal(got[b], want[b]), (b, r)
                if r[2] == 0.0:
                    assert torch.equal(got[b], one[b]), (b, r)


# ------------------------------------------------------------------------------------------------ c. the skip
@pytest.mark.parametrize("label,d,dtype", FEW)
def test_alpha_zero_never_reads_source_1(label, d, dtype):
    """Bank slot 2 is NaN and is named only as source 1, and only by rows whose alpha is 0: 0 x NaN = NaN, so a staged or read
    source 1 would poison those rows.  They are finite and equal the single-source launch on their source 0."""
    ops = _ops()
    B, heads, Tq, Tk = SHAPES[label]
    q, k, v, refs = _case(label, d, dtype, 3)
    qd, kd, vd = _up(q, dtype), _up(k, dtype).clone(), _up(ao.vt(v), dtype).clone()
    kd[2] = float("nan")
    vd[2] = float("nan")
    src, alpha, host = _table(B, [(0, 2, 0.0), (1, 2, 0.0), (0, 1, 0.3), (1, 2, 0.0)])
    got = ops.attention_bank(qd, kd, vd, src, alpha, heads)
    keep = [b for b, r in enumerate(host) if r[2] == 0.0]
    assert len(keep) >= 3 and torch.isfinite(got[keep]).all()
    for s0 in (0, 1):
        one = ops.attention(qd, kd[s0:s0 + 1], vd[s0:s0 + 1], heads)
        for b in keep:
            if host[b][0] == s0:
                assert torch.equal(got[b], one[b]), (b, host[b])
    blended = [b for b, r in enumerate(host) if r[2] != 0.0]
    _check(f"skip {label} d={d} {_name(dtype)} (the rows that blend two finite slots)", got[blended].float().cpu(),
           _blend(refs, host)[blended], dtype)


# ------------------------------------------------------------------------------------------------ d. the clamp
@pytest.mark.parametrize("label,d,dtype", FEW)
def test_indices_are_clamped_into_the_bank(label, d, dtype):
    """The bank is the middle S slots of an S + 2 slot allocation whose outer slots are NaN: an index of -1 or S that was not
    clamped would read them (inside the allocation: nothing out of bounds can happen).  -1 gives slot 0's result, S slot S - 1's."""
    ops = _ops()
    B, heads, Tq, Tk = SHAPES[label]
    S = 3
    q, k, v, _ = _case(label, d, dtype, S)
    C = heads * d
    kall = torch.full((S + 2, Tk, C), float("nan"), dtype=dtype, device="cuda")
    vall = torch.full((S + 2, C, Tk), float("nan"), dtype=dtype, device="cuda")
    kall[1:S + 1] = _up(k, dtype)
    vall[1:S + 1] = _up(ao.vt(v), dtype)
    kd, vd = kall[1:S + 1], vall[1:S + 1]
    assert kd.is_contiguous() and vd.is_contiguous() and kd.data_ptr() % 16 == 0 and vd.data_ptr() % 16 == 0
    qd = _up(q, dtype)
    big = 2 ** 31 - 1
    out_src, alpha, _ = _table(B, [(-1, S, 0.4), (S, -1, 0.6), (-big - 1, big, 0.25), (S, 1, 0.0), (-1, 1, 0.5)])
    in_src, _, _ = _table(B, [(0, S - 1, 0.4), (S - 1, 0, 0.6), (0, S - 1, 0.25), (S - 1, 1, 0.0), (0, 1, 0.5)])
    got = ops.attention_bank(qd, kd, vd, out_src, alpha, heads)
    want = ops.attention_bank(qd, kd, vd, in_src, alpha, heads)
    assert torch.isfinite(got).all() and torch.isfinite(want).all()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ e. guards and operands
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("label,d", [("w4-ragged", 24), ("w2-even", 8)])
def test_guards_column_slices_and_scale(label, d, dtype):
    """q is a column slice of a wider NaN-padded buffer (ldq = C + 8), k a column slice of a [S, Tk, 2C] buffer (as the fused
    projection leaves it), o sits between NaN guards that must survive, and the scale is not the default."""
    ops = _ops()
    B, heads, Tq, Tk = SHAPES[label]
    C = heads * d
    q, k, v, _ = _case(label, d, dtype, 3)
    refs = [ao.reference(q, k[s:s + 1], v[s:s + 1], heads, 0.37) for s in range(3)]
    qv, _ = ao.canary_wide(q, dtype, "cuda")
    kbuf = _up(torch.cat([torch.full_like(k, float("nan")), k], dim=2), dtype)
    kv = kbuf[:, :, C:]
    assert qv.stride(1) == C + 8 and kv.stride(1) == 2 * C
    out, whole = ao.canary((B, Tq, C), dtype, 64, "cuda")
    src, alpha, host = _table(B, ROWS)
    res = ops.attention_bank(qv, kv, _up(ao.vt(v), dtype), src, alpha, heads, scale=0.37, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    _check(f"guards {label} d={d} {_name(dtype)} scale=0.37", out.float().cpu(), _blend(refs, host), dtype)
    assert ao.guards_intact(whole, (B, Tq, C)), "the kernel wrote outside its output"
    default = [ao.reference(q, k[s:s + 1], v[s:s + 1], heads) for s in range(3)]
    assert ao.errors(_blend(refs, host), _blend(default, host))[0] > 1e-2          # (the scale reaches the oracle)


def test_graph_replay_reads_new_sources_and_weights():
    """src and alpha are read when the kernel runs: a captured launch replayed after the two tensors were rewritten gives the
    result of the new table."""
    ops = _ops()
    label, d, dtype = "w4-ragged", 24, BF16
    B, heads, Tq, Tk = SHAPES[label]
    q, k, v, _ = _case(label, d, dtype, 3)
    qd, kd, vd = _up(q, dtype), _up(k, dtype), _up(ao.vt(v), dtype)
    src, alpha, _ = _table(B, ROWS)
    out = torch.empty(B, Tq, heads * d, dtype=dtype, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention_bank(qd, kd, vd, src, alpha, heads, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.attention_bank(qd, kd, vd, src, alpha, heads, out=out)
    for rows in ([(2, 2, 0.0), (1, 0, 0.5)], [(0, 2, 0.9), (2, 1, 0.0), (1, 1, 0.2)]):
        s2, a2, _ = _table(B, rows)
        src.copy_(s2)
        alpha.copy_(a2)
        g.replay()
        assert torch.equal(out, ops.attention_bank(qd, kd, vd, s2, a2, heads)), rows


# ------------------------------------------------------------------------------------------------ f. refusals
def test_bank_refusals_leave_the_library_usable():
    from afldm_amd import _lib
    from afldm_amd._lib import AfldmError
    ops = _ops()

    def operands(dtype=BF16, B=3, S=2, heads=2, Tq=16, Tk=16, d=24):
        C = heads * d
        z = lambda *s: torch.zeros(*s, device="cuda", dtype=dtype)
        return [z(B, Tq, C), z(S, Tk, C), z(S, C, Tk), torch.zeros(B, 2, dtype=torch.int32, device="cuda"),
                torch.zeros(B, device="cuda"), heads]

    def wide_q(extra):
        a = operands()
        a[0] = torch.zeros(3, 16, 48 + extra, device="cuda", dtype=BF16)[:, :, :48]
        return a

    def shifted_q():
        a = operands()
        a[0] = torch.zeros(3 * 16 * 48 + 8, device="cuda", dtype=BF16)[4:4 + 3 * 16 * 48].view(3, 16, 48)
        return a

    def raw(a, S=None, src="keep", alpha="keep", src_offset=0):
        """the C entry point itself, for what the Python wrapper cannot express"""
        q, k, vt, s, al, heads = a
        B, Tq, C = q.shape
        out = torch.empty_like(q)
        sp = None if src is None else s.data_ptr() + src_offset
        ap = None if alpha is None else al.data_ptr()
        rc = _lib.lib.afldm_attention_bank(q.data_ptr(), C, k.data_ptr(), C, vt.data_ptr(), sp, ap, out.data_ptr(), C, B,
                                           k.shape[0] if S is None else S, heads, Tq, k.shape[1], C // heads, 0.2,
                                           _lib.DTYPE_CODE[q.dtype], _lib.stream_ptr())
        return rc, (_lib.lib.afldm_last_error() or b"").decode()

    def still_right(what):
        label, d, dtype = "w4-ragged", 24, BF16
        B, heads, Tq, Tk = SHAPES[label]
        q, k, v, refs = _case(label, d, dtype, 3)
        src, alpha, host = _table(B, ROWS)
        got = ops.attention_bank(_up(q, dtype), _up(k, dtype), _up(ao.vt(v), dtype), src, alpha, heads)
        _check(f"valid call after refusing {what}", got.float().cpu(), _blend(refs, host), dtype)

    assert raw(operands())[0] == 0
    for what, kw, match in (("S = 0", dict(S=0), "bank of S=0"), ("S = -1", dict(S=-1), "bank of S=-1"),
                            ("NULL src", dict(src=None), "NULL"), ("NULL alpha", dict(alpha=None), "NULL"),
                            ("src + 2 bytes", dict(src_offset=2), "4-byte aligned")):
        rc, msg = raw(operands(), **kw)
        assert rc != 0 and match in msg, (what, rc, msg)
        still_right(what)
    refused = [("bf16 Tk=12", operands(BF16, Tk=12), "Tk"), ("fp32 Tk=6", operands(F32, Tk=6), "Tk"),
               ("d=12", operands(BF16, d=12), "head_dim"), ("d=40", operands(F32, d=40), "head_dim"),
               ("ldq = C + 4", wide_q(4), "leading dims"), ("q + 4 elements", shifted_q(), "aligned")]
    for what, args, match in refused:
        with pytest.raises(AfldmError, match=match):
            ops.attention_bank(*args)
        still_right(what)
    ops.attention_bank(*wide_q(8))                                  # (the same placement is accepted once legal)
    # the wrapper's own checks: the shapes and dtypes attention_interp checks, for the bank's operands
    a = operands()
    for i, bad in ((3, a[3].long()), (3, a[3][:2]), (4, a[4].double()), (4, a[4][:2]), (2, a[2][:, :, :8].contiguous()), (2, a[2].float())):
        b = list(a)
        b[i] = bad
        with pytest.raises(ValueError, match="attention_bank"):
            ops.attention_bank(*b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attention_bank(*[t.cpu() if torch.is_tensor(t) else t for t in a])
