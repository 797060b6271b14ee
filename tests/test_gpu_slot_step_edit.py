"""afldm_slot_step_edit through ops on MI355X (afldm_amd/csrc/edit.hip, include/afldm_hip_edit.h): kinds 3 and 4 bit for bit
against the float32 restatement of tests/edit_oracle.py, the noises taken from afldm_counter_noise at the stated (ordinal, slot)
- tests/test_gpu_counter_noise.py pins that stream; kinds 0, 1 and 2 bit for bit against afldm_slot_step_seeded on the same
inputs; the 16-byte against the scalar form; what a held element, a NaN in the map, a zero coefficient and a slot that is not
to be touched do.

Shapes: B = 5, C = 4, 8 x 8 takes the 16-byte form, B = 3, C = 3, 5 x 3 the scalar one; both with fp32 and bf16 eps.  The table has
R = 16 rows of all five kinds and one unknown code."""
import math

import numpy as np
import pytest
import torch

import edit_oracle as eo
from test_gpu_slots import _bits

pytestmark = pytest.mark.gpu

INF = math.inf
SHAPES = [(5, 4, 8, 8), (3, 3, 5, 3)]
DTYPES = [torch.float32, torch.bfloat16]
# rows 0-2 "ddim" (c0, c1, c2, c3), 3-5 "dpm" (p, q, a, b0, b1, b2), 6-8 "seeded" (p, q, lo, hi, a, b, d, c),
# 9-11 "seeded_sdedit" (p, q, lo, hi, a, b, c, k0, k1, thr), 12-14 "seeded_repaint" (p, q, lo, hi, a, b, c, k0, k1, u0, u1), 15 unknown
ROWS = [[0.9, 0.43, 0.95, 0.31], [0.7, 0.71, 0.8, 0.6], [0.5, 0.86, 1.0, 0.0],
        [1.1, -0.4, 0.9, 0.3, 0.0, 0.0], [1.2, -0.5, 0.8, 0.45, -0.2, 0.0], [1.3, -0.6, 0.7, 0.5, -0.3, 0.1],
        [1.3, -0.7, -0.9, 1.1, 0.4, 0.8, 0.3, 0.6], [1.1, -0.5, -INF, INF, 0.0, 0.9, 0.2, 0.0], [1.05, -0.3, -INF, INF, 0.0, 0.95, 0.15, 0.3],
        [1.3, -0.7, -0.9, 1.1, 0.8, 0.3, 0.6, 0.85, 0.5, 0.45], [1.1, -0.5, -INF, INF, 0.9, 0.2, 0.0, 0.92, 0.38, 0.2],
        [1.02, -0.2, -INF, INF, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0],
        [1.3, -0.7, -0.9, 1.1, 0.8, 0.3, 0.6, 0.85, 0.5, 0.93, 0.36], [1.1, -0.5, -INF, INF, 0.9, 0.2, 0.0, 0.92, 0.38, 1.0, 0.0],
        [1.02, -0.2, -INF, INF, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0],
        [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]]
KIND = [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3 + [7]
ORD = [0, 1, 2, 0, 1, 2, 4, 5, 6, 3, 17, 49, 0, 8, 9, 1]
R = 16
SEEDS = [3, (1 << 62) + 11, 12345, 0, 99]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def _table(width=12):
    rows = [list(r)[:width] + [0.0] * (width - min(len(r), width)) for r in ROWS]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


def _inputs(shape, dtype, seed=6):
    """(x, eps NHWC, hist, cond, cmask) on the host; the map holds exact 0s and 1s, values on both sides of every thr, and soft ones."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    eps = torch.randn(B, H, W, C, generator=g).to(dtype)
    hist = torch.randn(2, B, C, H, W, generator=g)
    cond = torch.randn(B, C, H, W, generator=g)
    cmask = torch.rand(B, 1, H, W, generator=g)
    cmask.reshape(B, -1)[:, 0::5] = 0.0
    cmask.reshape(B, -1)[:, 1::5] = 1.0
    return x, eps, hist, cond, cmask


def _run(x, eps, hist, cond, cmask, pos, active, seeds, table=None, kind=None):
    """One launch on device copies: (x, hist) afterwards."""
    from afldm_amd import ops
    B = x.shape[0]
    xd, hd = x.cuda(), hist.cuda()
    out = ops.slot_step_edit(xd, eps.cuda(), hd, cond.cuda(), cmask.cuda(), (_table() if table is None else table).cuda(),
                             _i32(KIND if kind is None else kind), _i32(ORD), _i32(pos), _i32(active), _i64(seeds[:B]))
    assert out is xd
    return xd, hd


def _device_noise(shape):
    """noise(seed, ordinal, slot) for edit_oracle.slot_step: afldm_counter_noise's values of one sample."""
    from afldm_amd import ops

    def noise(seed, ordinal, slot):
        return ops.counter_noise(_i64([seed]), _i32([ordinal]), (1,) + tuple(shape[1:]), slot=slot)[0].cpu().numpy()
    return noise


def _want(x, eps, cond, cmask, pos, active, seeds, table=None, kind=None):
    e = eps.float().permute(0, 3, 1, 2).contiguous().numpy()
    return eo.slot_step(x.numpy(), e, cond.numpy(), cmask.numpy(), (_table() if table is None else table).double().numpy(),
                        KIND if kind is None else kind, ORD, pos, active, seeds, _device_noise(x.shape))


# ------------------------------------------------------------------------------------------------ 1. kinds 3 and 4
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kinds_3_and_4_bit_for_bit(shape, dtype):
    B = shape[0]
    x, eps, hist, cond, cmask = _inputs(shape, dtype)
    hist[:] = float("nan")                                               # kinds 3 and 4 neither read nor write it
    table = _table()
    for first in range(9, 15):
        pos = [9 + (first - 9 + b) % 6 for b in range(B)]                # every slot on another edit row, each row in each slot's place
        got, h = _run(x, eps, hist, cond, cmask, pos, [1] * B, SEEDS)
        want = _want(x, eps, cond, cmask, pos, [1] * B, SEEDS)
        assert np.array_equal(_bits(got).numpy(), want.view(np.int32)), (first, shape, dtype)
        assert torch.isfinite(got).all() and torch.equal(_bits(h), _bits(hist)) and not torch.equal(got.cpu(), x)
    e = eps.float().permute(0, 3, 1, 2)
    t = table[9, 0] * x + table[9, 1] * e
    assert ((t < table[9, 2]) | (t > table[9, 3])).any() and ((t > table[9, 2]) & (t < table[9, 3])).any(), "the clamp is active"
    for r in (9, 10, 11):
        held = cmask <= table[r, 9]
        assert held.any() and (~held).any(), r
    # the last rows return the conditioning exactly: the original where the map is 0, the known latents where the mask is 1
    got, _ = _run(x, eps, hist, cond, cmask, [11] * B, [1] * B, SEEDS)
    zero = (cmask == 0).expand_as(cond)
    assert torch.equal(got.cpu()[zero], cond[zero]) and zero.any()
    got, _ = _run(x, eps, hist, cond, cmask, [14] * B, [1] * B, SEEDS)
    one = (cmask == 1).expand_as(cond)
    assert torch.equal(got.cpu()[one], cond[one]) and one.any()


def test_a_request_s_noise_is_its_seed_s_and_its_ordinal_s():
    """Four slots with the same inputs: the same seed gives the same update, another seed or another ordinal another one."""
    x, eps, hist, cond, cmask = (t.repeat_interleave(4, dim=t.dim() - 4) for t in _inputs((1, 4, 8, 8), torch.float32))
    for row in (9, 12):
        table, kind = _table(), list(KIND)
        table[15], kind[15] = table[row], kind[row]                      # row 15: the same row at another ordinal
        assert ORD[15] != ORD[row]
        got, _ = _run(x, eps, hist, cond, cmask, [row, row, row, 15], [1] * 4, [7, 7, 8, 7], table, kind)
        assert torch.equal(got[0], got[1]) and not torch.equal(got[0], got[2]) and not torch.equal(got[0], got[3]), row
    # "seeded_sdedit": the fixed noise z does not move with the ordinal - a row with c = 0 gives the same update at both
    table, kind = _table(), list(KIND)
    table[15], kind[15] = table[10], 3
    got, _ = _run(x, eps, hist, cond, cmask, [10, 15, 10, 15], [1] * 4, [7, 7, 8, 8], table, kind)
    assert float(table[10, 6]) == 0.0 and float(table[10, 8]) != 0.0 and ORD[15] != ORD[10]
    assert torch.equal(got[0], got[1]) and torch.equal(got[2], got[3]) and not torch.equal(got[0], got[2])


# ------------------------------------------------------------------------------------------------ 2. kinds 0, 1 and 2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kinds_0_1_and_2_have_slot_step_seeded_bits(shape, dtype):
    from afldm_amd import ops
    B = shape[0]
    x, eps, hist, cond, cmask = _inputs(shape, dtype, seed=7)
    cond[:], cmask[:] = float("nan"), float("nan")                       # never read by these kinds
    narrow = _table(8)
    assert torch.equal(narrow, _table()[:, :8])
    for first in range(9):
        pos = [(first + 2 * b) % 9 for b in range(B)]
        got_x, got_h = _run(x, eps, hist, cond, cmask, pos, [1] * B, SEEDS)
        want_x, want_h = x.cuda(), hist.cuda()
        ops.slot_step_seeded(want_x, eps.cuda(), want_h, narrow.cuda(), _i32(KIND), _i32(ORD), _i32(pos), _i32([1] * B), _i64(SEEDS[:B]))
        assert torch.equal(_bits(got_x), _bits(want_x)) and torch.equal(_bits(got_h), _bits(want_h)), (first, shape, dtype)
        assert not torch.equal(got_x.cpu(), x) and torch.isfinite(got_x).all()
        if any(KIND[p] == 1 for p in pos):
            assert not torch.equal(got_h.cpu(), hist)


# ------------------------------------------------------------------------------------------------ 3. the two forms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["x", "hist", "cond", "cmask"])
def test_the_16_byte_and_the_scalar_form_agree(which, dtype):
    """One of the four fp32 tensors on a base offset by one float takes the scalar form: the same bits for kinds 0, 2, 3 and 4.  A
    "dpm" slot has afldm_dpm_step's bits, whose two forms differ by design (slot_common.hpp): it is compared with
    afldm_slot_step_seeded in the same form instead."""
    from afldm_amd import ops
    shape = SHAPES[0]
    B = shape[0]
    host = dict(zip(("x", "eps", "hist", "cond", "cmask"), _inputs(shape, dtype, seed=8)))
    for pos in ([0, 4, 8, 9, 12], [13, 10, 6, 5, 2], [14, 11, 7, 3, 1]):
        wide_x, wide_h = _run(host["x"], host["eps"], host["hist"], host["cond"], host["cmask"], pos, [1] * B, SEEDS)
        dev = {k: v.cuda() for k, v in host.items()}
        buf = torch.full((host[which].numel() + 2,), 9.0, device="cuda")
        dev[which] = buf[1:-1].view(host[which].shape)
        dev[which].copy_(host[which])
        assert dev[which].data_ptr() % 16 == 4 and dev[which].is_contiguous()
        ref_x, ref_h = dev["x"].clone(), dev["hist"].clone()             # (clones are aligned: the 16-byte form of the sibling)
        if which in ("x", "hist"):
            off = torch.full((host[which].numel() + 2,), 9.0, device="cuda")[1:-1].view(host[which].shape)
            off.copy_(host[which])
            ref_x, ref_h = (off, ref_h) if which == "x" else (ref_x, off)
            ops.slot_step_seeded(ref_x, dev["eps"], ref_h, _table(8).cuda(), _i32(KIND), _i32(ORD), _i32(pos), _i32([1] * B), _i64(SEEDS))
        ops.slot_step_edit(dev["x"], dev["eps"], dev["hist"], dev["cond"], dev["cmask"], _table().cuda(), _i32(KIND), _i32(ORD),
                           _i32(pos), _i32([1] * B), _i64(SEEDS))
        for b in range(B):
            same = torch.equal(_bits(dev["x"][b]), _bits(wide_x[b])) and torch.equal(_bits(dev["hist"][:, b]), _bits(wide_h[:, b]))
            if KIND[pos[b]] != 1:
                assert same, (which, pos, b, KIND[pos[b]])
            if KIND[pos[b]] <= 2 and which in ("x", "hist"):
                assert torch.equal(_bits(dev["x"][b]), _bits(ref_x[b])) and torch.equal(_bits(dev["hist"][:, b]), _bits(ref_h[:, b])), \
                    (which, pos, b, "against afldm_slot_step_seeded in the scalar form")
        assert float(buf[0]) == 9.0 and float(buf[-1]) == 9.0


# ------------------------------------------------------------------------------------------------ 4. NaN, Inf and zero coefficients
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_held_elements_nan_maps_and_zero_coefficients(shape, dtype):
    B = shape[0]
    x, eps, hist, cond, cmask = _inputs(shape, dtype, seed=9)
    clean, _ = _run(x, eps, hist, cond, cmask, [9] * B, [1] * B, SEEDS)
    # held elements (map <= thr) ignore NaN in x and Inf in eps: a select, not a blend
    held = (cmask <= _table()[9, 9]).expand_as(x)
    xn, en = x.clone(), eps.float().permute(0, 3, 1, 2).clone()
    xn[held], en[held] = float("nan"), float("inf")
    en = en.permute(0, 2, 3, 1).contiguous().to(dtype)
    got, _ = _run(xn, en, hist, cond, cmask, [9] * B, [1] * B, SEEDS)
    assert torch.equal(_bits(got), _bits(clean)) and torch.isfinite(got).all() and held.any() and (~held).any()
    # released elements take nothing of the original: NaN there does not reach them
    cn = cond.clone()
    cn[~held] = float("nan")
    got, _ = _run(x, eps, hist, cn, cmask, [9] * B, [1] * B, SEEDS)
    assert torch.equal(_bits(got), _bits(clean))
    # a NaN in the change map compares false: the element is generated, as one of map value 1 is
    mn, m1 = cmask.clone(), cmask.clone()
    mn[:, :, 0, :], m1[:, :, 0, :] = float("nan"), 1.0
    got, _ = _run(x, eps, hist, cond, mn, [9] * B, [1] * B, SEEDS)
    as_one, _ = _run(x, eps, hist, cond, m1, [9] * B, [1] * B, SEEDS)
    assert torch.equal(_bits(got), _bits(as_one)) and torch.isfinite(got).all() and float(_table()[9, 9]) < 1.0
    assert np.array_equal(_bits(got).numpy(), _want(x, eps, cond, mn, [9] * B, [1] * B, SEEDS).view(np.int32))
    # history planes behind a zero coefficient may hold NaN: "dpm" rows with b1 = b2 = 0 (h1 is shifted, not used) and b2 = 0
    hn = hist.clone()
    hn[1] = float("nan")
    got, h = _run(x, eps, hn, cond, cmask, [4] * B, [1] * B, SEEDS)
    assert torch.isfinite(got).all() and torch.isfinite(h).all(), "b2 = 0: h2 is not read, and is overwritten by h1"
    hn[0] = float("nan")
    got, h = _run(x, eps, hn, cond, cmask, [3] * B, [1] * B, SEEDS)
    assert torch.isfinite(got).all() and torch.isfinite(h[0]).all() and torch.isnan(h[1]).all()
    # a noise behind a zero coefficient is not generated: rows 10 / 11 / 13 / 14 equal the oracle, which then never asks for it
    for row, fields in ((10, (6,)), (11, (6, 8)), (13, (6, 10)), (14, (6, 8, 10))):
        assert all(float(_table()[row, f]) == 0.0 for f in fields)
        got, _ = _run(x, eps, hist, cond, cmask, [row] * B, [1] * B, SEEDS)
        assert np.array_equal(_bits(got).numpy(), _want(x, eps, cond, cmask, [row] * B, [1] * B, SEEDS).view(np.int32)), row


# ------------------------------------------------------------------------------------------------ 5. slots that are not touched
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_inactive_out_of_range_and_unknown_slots_are_untouched(shape, dtype):
    B = shape[0]
    x, eps, hist, cond, cmask = _inputs(shape, dtype, seed=10)
    cases = [([9, 12, 3], [0, 0, 0]), ([R, -3, 2 ** 31 - 1], [1, 1, 1]), ([15, 15, -1], [1, 1, 1])]
    x[:, 0, 0, 0] = float("nan")
    eps[:] = float("nan")
    for pos, active in cases:
        pos, active = (pos * 2)[:B], (active * 2)[:B]
        got, h = _run(x, eps, hist, cond, cmask, pos, active, SEEDS)
        assert torch.equal(_bits(got), _bits(x)) and torch.equal(_bits(h), _bits(hist)), pos
    # one live slot among them is updated, and it alone
    x2, eps2, _, _, _ = _inputs(shape, dtype, seed=11)
    pos, active = ([12, R, 9] * 2)[:B], ([1, 1, 0] * 2)[:B]
    got, h = _run(x2, eps2, hist, cond, cmask, pos, active, SEEDS)
    want = _want(x2, eps2, cond, cmask, pos, active, SEEDS)
    live = [b for b in range(B) if pos[b] == 12]
    assert np.array_equal(_bits(got).numpy(), want.view(np.int32)) and torch.equal(_bits(h), _bits(hist))
    assert all(not torch.equal(got[b].cpu(), x2[b]) for b in live) and all(torch.equal(got[b].cpu(), x2[b]) for b in range(B) if b not in live)
