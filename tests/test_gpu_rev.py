"""The bit-reversible sampler's kernels on MI355X (afldm_rev_step, afldm_rev_step_flat, afldm_rev_encode) against the numpy oracle
of tests/rev_oracle.py, bit for bit: torch.equal on far, near, lat and bad.  Shapes: an odd element count (the scalar path, C = 3
in the NHWC gather), the 16-byte path, a misaligned slice that falls back to the scalar path, and more elements than a smaller
grid cap would cover in one pass.  Planted states test the int64 -> fp32 ties and the large magnitudes; planted eps the trouble
flags, per sample."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import rev_oracle as ro

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SHAPES = [(3, 3, 5, 5), (2, 4, 8, 8), (1, 4, 8, 8), (70, 4, 16, 16)]          # the third is given misaligned
PLANT = [0, 1, -1, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, -(2 ** 24 + 3), 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 62, -(2 ** 62)]
I64_GUARD, I32_GUARD = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
PAD = 64
OK, ESHAPE, EDTYPE, EALIGN, ENULL = 0, -1, -2, -3, -5


def guarded(t, shift=0):
    """t on the device inside a larger buffer of guard values (NaN for floats): (buffer, view).  shift: elements by which the
    view starts off the 512-byte aligned position."""
    guard = {torch.int64: I64_GUARD, torch.int32: I32_GUARD}.get(t.dtype, float("nan"))
    buf = torch.full((t.numel() + 2 * PAD,), guard, dtype=t.dtype, device="cuda")
    view = buf[PAD + shift:PAD + shift + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def guards_intact(buf, view, shift=0):
    n = view.numel()
    edge = torch.cat([buf[:PAD + shift], buf[PAD + shift + n:]])
    return bool(torch.isnan(edge).all()) if buf.is_floating_point() else bool((edge == edge[0]).all()) and int(edge[0]) in (I64_GUARD, I32_GUARD)


def states(shape, seed):
    """(far, near) int64: random within +-2^34 (latents of magnitude <= 4), the planted values at the head of near, then of far."""
    g = torch.Generator().manual_seed(seed)
    far = torch.randint(-2 ** 34, 2 ** 34, shape, generator=g, dtype=torch.int64)
    near = torch.randint(-2 ** 34, 2 ** 34, shape, generator=g, dtype=torch.int64)
    p = torch.tensor(PLANT, dtype=torch.int64)
    near.view(-1)[:len(PLANT)] = p
    far.view(-1)[len(PLANT):2 * len(PLANT)] = p
    return far, near


def eps_of(shape, dtype, seed):
    """eps NCHW fp32 holding values of `dtype`, and the NHWC device tensor the kernel reads."""
    e = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).float()
    return e, e.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)


def table(sign, boot, seed=5):
    """Three rows; the middle one is the row under test.  |cx|, |ce| <= 0.9: the planted +-2^62 then stay inside int64, also
    doubled by a boot row, so that nothing but what a test plants is trouble."""
    c = torch.randn(3, 4, generator=torch.Generator().manual_seed(seed)).clamp_(-0.9, 0.9)
    c[:, 2] = torch.tensor([-sign, sign, -sign], dtype=torch.float32)
    c[:, 3] = torch.tensor([1 - boot, boot, 1 - boot], dtype=torch.float32)
    return c


def launch(far, near, e_dev, row_table, shape, shift=0, idx=1, advance=True):
    """One afldm_rev_step on guarded buffers: (far, near, lat, bad, idx) as CPU tensors, after checking every guard."""
    from afldm_amd import ops
    fb, fv = guarded(far, shift)
    nb, nv = guarded(near, shift)
    lb, lv = guarded(torch.zeros(shape), shift)
    bb, bv = guarded(torch.zeros(shape[0], dtype=torch.int32))
    step = torch.full((1,), idx, dtype=torch.int32, device="cuda")
    out = ops.rev_step(fv, nv, e_dev, bv, row_table.cuda().reshape(-1).contiguous(), step, advance=advance, out=lv)
    torch.cuda.synchronize()
    assert out is lv
    assert guards_intact(fb, fv, shift) and guards_intact(nb, nv, shift) and guards_intact(lb, lv, shift) and guards_intact(bb, bv)
    return fv.cpu(), nv.cpu(), lv.cpu(), bv.cpu(), int(step.item())


def want_step(far, near, e, row, B):
    f, n, lat, bad = ro.step(far.numpy(), near.numpy(), e.numpy(), (float(row[0]), float(row[1]), int(row[2]), int(row[3])))
    return (torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(lat),
            torch.from_numpy(bad.reshape(B, -1).any(axis=1).astype(np.int32)))


def same(got, want):
    return all(torch.equal(g, w) for g, w in zip(got[:4], want))


@pytest.mark.parametrize("dtype,shape,boot,sign", list(itertools.product(DTYPES, SHAPES, (0, 1), (1, -1))))
def test_rev_step_kernel(dtype, shape, boot, sign):
    shift = 1 if shape == (1, 4, 8, 8) else 0                          # 8 bytes off: int64-aligned, not 16-byte aligned
    far, near = states(shape, 7)
    e, e_dev = eps_of(shape, dtype, 8)
    tb = table(sign, boot)
    got = launch(far, near, e_dev, tb, shape, shift)
    want = want_step(far, near, e, tb[1], shape[0])
    assert got[4] == 2                                                 # advance
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "far / near"
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]), "lat / bad"
    assert not want[3].any() and torch.equal(got[0], near)             # the rotation; no trouble on these values
    assert not torch.equal(got[1], far if not boot else near)
    # the planted states decode as the oracle says (ties to even at 2^24 + 1 and + 3, one rounding at 2^53 + 1)
    from afldm_amd.reversible import decode
    assert torch.equal(decode(near.cuda()).cpu(), torch.from_numpy(ro.decode(near.numpy())))


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, SHAPES[:2])))
def test_trouble_is_flagged_per_sample_and_leaves_the_others_alone(dtype, shape):
    B = shape[0]
    per = shape[1] * shape[2] * shape[3]
    far, near = states(shape, 11)
    e, _ = eps_of(shape, dtype, 12)
    tb = table(1, 0)
    tb[1, :2] = torch.tensor([0.7, 1.3])
    clean = want_step(far, near, e, tb[1], B)
    assert not clean[3].any()
    big = float(torch.tensor(4.0e9).to(dtype))                         # 1.3 * 4e9 >= 2^31: d is finite, d 2^32 >= 2^63
    for b, value in ((1, float("nan")), (B - 1, float("inf")), (0, -float("inf")), (1, big), (0, "overflow")):
        f2, n2, e2 = far.clone(), near.clone(), e.clone()
        at = b * per + per // 2 + 1
        if value == "overflow":
            f2.view(-1)[at], n2.view(-1)[at] = 2 ** 63 - 5, 2 ** 40       # x = 2^8: q ~ 179 * 2^32 > 5
        else:
            e2.view(-1)[at] = value
        e_dev = e2.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)
        got = launch(f2, n2, e_dev, tb, shape)
        want = want_step(f2, n2, e2, tb[1], B)
        assert same(got, want), (b, value)
        flags = [int(i == b) for i in range(B)]
        assert got[3].tolist() == flags, (b, value, got[3].tolist())
        assert int(got[1].view(-1)[at]) == int(f2.view(-1)[at])         # q = 0: new = f
        keep = torch.ones(B * per, dtype=torch.bool)
        keep[at] = False
        assert torch.equal(got[1].view(-1)[keep], clean[1].view(-1)[keep])          # every other element as in a clean run
        assert torch.equal(got[2].view(-1)[keep], clean[2].view(-1)[keep])


@pytest.mark.parametrize("dtype,shape", list(itertools.product(DTYPES, SHAPES[:3])))
def test_step_then_its_inverse_restores_both_tensors(dtype, shape):
    from afldm_amd import ops
    shift = 1 if shape == (1, 4, 8, 8) else 0
    far, near = states(shape, 21)
    e, e_dev = eps_of(shape, dtype, 22)
    for sign in (1, -1):
        _, fv = guarded(far, shift)
        _, nv = guarded(near, shift)
        bad = torch.zeros(shape[0], dtype=torch.int32, device="cuda")
        lat = torch.empty(shape, device="cuda")
        step = torch.ones(1, dtype=torch.int32, device="cuda")
        ops.rev_step(fv, nv, e_dev, bad, table(sign, 0).cuda().reshape(-1), step, out=lat)
        assert torch.equal(fv.cpu(), near) and not torch.equal(nv.cpu(), far)
        # the same row with the opposite sign, fed the rotated pair: far := the new state, near := the state eps belongs to
        ops.rev_step(nv, fv, e_dev, bad, table(-sign, 0).cuda().reshape(-1), step, out=lat)
        assert torch.equal(fv.cpu(), far) and torch.equal(nv.cpu(), near) and not bad.any()
        assert torch.equal(lat.cpu(), torch.from_numpy(ro.decode(far.numpy())))


def test_captured_launch_follows_rewritten_coef_and_step_idx():
    from afldm_amd import ops
    shape = (2, 4, 8, 8)
    far, near = states(shape, 31)
    e, e_dev = eps_of(shape, torch.bfloat16, 32)
    fv, nv = far.cuda(), near.cuda()
    bad = torch.zeros(2, dtype=torch.int32, device="cuda")
    lat = torch.zeros(shape, device="cuda")
    coef = table(1, 0).cuda().reshape(-1).contiguous()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rev_step(fv, nv, e_dev, bad, coef, step, advance=True, out=lat)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.rev_step(fv, nv, e_dev, bad, coef, step, advance=True, out=lat)
    # everything the graph reads is rewritten behind its back: the pair, the table, the counter
    tb = table(-1, 0, seed=77)
    tb[2, 2:] = torch.tensor([1.0, 1.0])
    fv.copy_(far); nv.copy_(near); bad.zero_(); coef.copy_(tb.reshape(-1)); step.fill_(1)
    g.replay()
    torch.cuda.synchronize()
    w1 = want_step(far, near, e, tb[1], 2)
    assert same((fv.cpu(), nv.cpu(), lat.cpu(), bad.cpu()), w1) and int(step.item()) == 2
    g.replay()                                                           # the counter advanced: the next row, a boot row
    torch.cuda.synchronize()
    w2 = want_step(w1[0], w1[1], e, tb[2], 2)
    assert same((fv.cpu(), nv.cpu(), lat.cpu(), bad.cpu()), w2) and int(step.item()) == 3


@pytest.mark.parametrize("shape,shift", [((3, 3, 5, 5), 0), ((2, 4, 8, 8), 0), ((1, 4, 8, 8), 1), ((5, 7), 0)])
def test_flat_form_is_the_table_form_bit_for_bit(shape, shift):
    from afldm_amd import ops
    far, near = states(shape, 41)
    e = torch.randn(shape, generator=torch.Generator().manual_seed(42))
    e.view(-1)[3] = float("nan")                                         # trouble in sample 0, in both forms
    for sign, boot in itertools.product((1, -1), (0, 1)):
        tb = table(sign, boot)
        row = (float(tb[1, 0]), float(tb[1, 1]), sign, boot)
        fb, fv = guarded(far, shift)
        nb, nv = guarded(near, shift)
        lb, lv = guarded(torch.zeros(shape), shift)
        bb, bv = guarded(torch.zeros(shape[0], dtype=torch.int32))
        assert ops.rev_step_flat(fv, nv, e.cuda(), bv, row, out=lv) is lv
        torch.cuda.synchronize()
        assert guards_intact(fb, fv, shift) and guards_intact(nb, nv, shift) and guards_intact(lb, lv, shift) and guards_intact(bb, bv)
        flat = (fv.cpu(), nv.cpu(), lv.cpu(), bv.cpu())
        assert same(flat, want_step(far, near, e, row, shape[0])) and flat[3].tolist() == [1] + [0] * (shape[0] - 1)
        if len(shape) == 4:
            got = launch(far, near, e.permute(0, 2, 3, 1).contiguous().cuda(), tb, shape, shift)
            assert same(got, flat), (sign, boot)
    # one buffer for far and near: a boot row takes it and leaves the new state there
    one = near.cuda()
    bad = torch.zeros(shape[0], dtype=torch.int32, device="cuda")
    e2 = torch.randn(shape, generator=torch.Generator().manual_seed(43))
    ops.rev_step_flat(one, one, e2.cuda(), bad, (0.5, -0.25, 1, 1))
    assert torch.equal(one.cpu(), want_step(near, near, e2, (0.5, -0.25, 1, 1), shape[0])[1]) and not bad.any()


def test_rev_encode():
    from afldm_amd import ops
    heads = [0.0, 2.0 ** -33, -2.0 ** -33, 2.0 ** 31 - 2.0 ** 7, -(2.0 ** 31 - 2.0 ** 7), 2.0 ** 31, -2.0 ** 31, float("nan"),
             float("inf"), 3 * 2.0 ** -33]
    x = torch.randn(len(heads), 37, generator=torch.Generator().manual_seed(51))
    x[:, 0] = torch.tensor(heads)
    Xb, Xv = guarded(torch.zeros(x.shape, dtype=torch.int64))
    bb, bv = guarded(torch.zeros(len(heads), dtype=torch.int32))
    assert ops.rev_encode(x.cuda(), bv, out=Xv) is Xv
    torch.cuda.synchronize()
    assert guards_intact(Xb, Xv) and guards_intact(bb, bv)
    X, bad = ro.encode(x.numpy())
    assert torch.equal(Xv.cpu(), torch.from_numpy(X))
    assert bv.cpu().tolist() == bad.any(axis=1).astype(int).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0]
    assert Xv[:, 0].cpu().tolist() == [0, 0, 0, (2 ** 31 - 2 ** 7) << 32, -((2 ** 31 - 2 ** 7) << 32), 0, 0, 0, 0, 2]
    # a value of the grid survives encode -> decode -> encode
    from afldm_amd.reversible import decode
    y = decode(Xv)
    again = ops.rev_encode(y.contiguous(), torch.zeros(len(heads), dtype=torch.int32, device="cuda"))
    assert torch.equal(decode(again), y)


def test_refusals_leave_the_library_usable():
    from afldm_amd import ops
    from afldm_amd._lib import lib, ptr, stream_ptr
    shape = (2, 4, 8, 8)
    far, near = states(shape, 61)
    e, e_dev = eps_of(shape, torch.float32, 62)
    fv, nv = far.cuda(), near.cuda()
    lat = torch.full(shape, 7.0, device="cuda")
    bad = torch.zeros(2, dtype=torch.int32, device="cuda")
    coef = table(1, 0).cuda().reshape(-1).contiguous()
    step = torch.ones(1, dtype=torch.int32, device="cuda")
    st = stream_ptr()
    args = [ptr(fv), ptr(nv), ptr(e_dev), ptr(lat), ptr(bad), ptr(coef), ptr(step)]

    def step_rc(a, dims=(2, 4, 8, 8), dtype=0):
        return lib.afldm_rev_step(*a, 1, *dims, dtype, st)

    for i in range(7):
        assert step_rc(args[:i] + [None] + args[i + 1:]) == ENULL, i
    assert b"afldm_rev_step" in lib.afldm_last_error()
    assert step_rc(args, dims=(2, 0, 8, 8)) == ESHAPE and step_rc(args, dtype=9) == EDTYPE
    assert step_rc([args[0] + 4] + args[1:]) == EALIGN and step_rc([args[0], args[1] + 4] + args[2:]) == EALIGN
    assert step_rc([args[0], args[0]] + args[2:]) == ESHAPE and b"one buffer" in lib.afldm_last_error()
    flat = [ptr(fv), ptr(nv), ptr(e.cuda()), ptr(lat), ptr(bad)]
    n = far.numel()

    def flat_rc(a, sign=1, boot=0, n=n, per=n // 2):
        return lib.afldm_rev_step_flat(*a, 0.5, 0.5, sign, boot, n, per, st)

    for i in range(5):
        assert flat_rc(flat[:i] + [None] + flat[i + 1:]) == ENULL, i
    assert flat_rc(flat, sign=0) == ESHAPE and flat_rc(flat, sign=2) == ESHAPE and flat_rc(flat, per=0) == ESHAPE
    assert flat_rc([flat[0] + 4] + flat[1:]) == EALIGN
    assert flat_rc([flat[0], flat[0]] + flat[2:]) == ESHAPE              # one buffer without boot
    assert flat_rc(flat, n=0) == OK
    X = torch.zeros(8, dtype=torch.int64, device="cuda")
    x = torch.zeros(8, device="cuda")
    assert lib.afldm_rev_encode(None, ptr(X), ptr(bad), 8, 4, st) == ENULL and lib.afldm_rev_encode(ptr(x), None, ptr(bad), 8, 4, st) == ENULL
    assert lib.afldm_rev_encode(ptr(x), ptr(X), None, 8, 4, st) == ENULL and lib.afldm_rev_encode(ptr(x), ptr(X), ptr(bad), 8, 0, st) == ESHAPE
    assert lib.afldm_rev_encode(ptr(x), ptr(X) + 4, ptr(bad), 4, 4, st) == EALIGN and lib.afldm_rev_encode(ptr(x), ptr(X), ptr(bad), 0, 4, st) == OK
    torch.cuda.synchronize()
    # nothing was launched: every tensor is as it was
    assert torch.equal(fv.cpu(), far) and torch.equal(nv.cpu(), near) and bool((lat == 7.0).all()) and not bad.any() and int(step.item()) == 1
    # the wrappers
    with pytest.raises(ValueError):
        ops.rev_step(fv.int(), nv, e_dev, bad, coef, step)
    with pytest.raises(ValueError):
        ops.rev_step(fv, nv[:1], e_dev, bad, coef, step)
    with pytest.raises(ValueError):
        ops.rev_step(fv, nv, e.cuda(), bad, coef, step)                  # eps not NHWC
    with pytest.raises(ValueError):
        ops.rev_step(fv, nv, e_dev, bad[:1], coef, step)
    with pytest.raises(ValueError):
        ops.rev_step(fv, nv, e_dev, bad, coef, step, out=lat.double())
    with pytest.raises(RuntimeError, match="one buffer"):
        ops.rev_step(fv, fv, e_dev, bad, coef, step)
    with pytest.raises(ValueError):
        ops.rev_step_flat(fv, nv, e.cuda(), bad, (0.5, 0.5, 0, 0))
    with pytest.raises(ValueError):
        ops.rev_step_flat(fv, nv, e.cuda().double(), bad, (0.5, 0.5, 1, 0))
    with pytest.raises(ValueError):
        ops.rev_encode(x.double(), bad)
    with pytest.raises(ValueError):
        ops.rev_encode(x.reshape(2, 4), bad[:1])
    with pytest.raises(RuntimeError, match="fp32 / bf16"):
        ops.rev_step(fv, nv, e_dev.half(), bad, coef, step)
    # and the library still computes
    got = ops.rev_step(fv, nv, e_dev, bad, coef, step, out=lat)
    want = want_step(far, near, e, table(1, 0)[1], 2)
    assert same((fv.cpu(), nv.cpu(), got.cpu(), bad.cpu()), want)
