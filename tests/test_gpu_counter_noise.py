"""libafldm_noise.so through ops on MI355X (afldm_amd/csrc/noise.hip, include/afldm_hip_noise.h): the Philox words against the
Random123 known answers and tests/noise_oracle.py, the normals against the float64 oracle, afldm_seeded_step bit for bit against
the float32 restatement of its update on afldm_counter_noise's own output, and afldm_slot_step_seeded against
afldm_slot_step_kinds (kinds 0 and 1) and afldm_seeded_step (kind 2).

Accuracy of the normals: the bound is 4 x E32 max-abs, E32 being what the numpy float32 evaluation of the same formula loses
against float64 on the same counters (the test computes it); the factor 4 allows the device's log / sincos a few ulp against
the host's.  Measured on MI355X, seed 12345, ordinal 3, 2^20 values: device 6.555e-07, E32 1.596e-06 (DESIGN.md section 28;
profiles/seeded/test_gpu_counter_noise.log)."""
import math

import numpy as np
import pytest
import torch

import noise_oracle as no
from test_counter_noise_host import KNOWN, check_cross, check_moments
from test_gpu_slots import R, SPANS, T, _bits
from test_gpu_slots_dpm import DDIM, DPM, _states, _tables

pytestmark = pytest.mark.gpu


def _i64(values):
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in values], dtype=torch.int64, device="cuda")


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the words
def test_philox_known_answers():
    from afldm_amd import ops
    for counter, key, want in KNOWN:
        got = ops.philox_bits(_i64([key[0] | (key[1] << 32)]), 1, g0=counter[0], ordinal=counter[1], slot=counter[2], c3=counter[3])
        assert tuple(got.shape) == (1, 1, 4) and [int(v) for v in _u32(got).reshape(-1)] == list(want)


@pytest.mark.parametrize("groups", [1, 5, 2048 * 256 + 3])              # the last: past the grid cap, the grid-stride loop
def test_philox_bits_against_the_oracle(groups):
    from afldm_amd import ops
    seeds = [0, 12345, (1 << 63) - 1]
    g0 = 0xfffffffe if groups == 5 else 7                                # (the group index wraps modulo 2^32)
    got = _u32(ops.philox_bits(_i64(seeds), groups, g0=g0, ordinal=3, slot=1, c3=0))
    for b, seed in enumerate(seeds):
        assert np.array_equal(got[b], no.words(seed, groups, g0, 3, 1, 0)), (b, seed)
    # an unaligned output: the scalar stores
    buf = torch.zeros(3 * min(groups, 64) * 4 + 1, dtype=torch.int32, device="cuda")
    out = buf[1:].view(3, min(groups, 64), 4)
    ops.philox_bits(_i64(seeds), min(groups, 64), g0=g0, ordinal=3, slot=1, out=out)
    assert np.array_equal(_u32(out), got[:, :min(groups, 64)]) and int(buf[0]) == 0


# ------------------------------------------------------------------------------------------------ 2. the normals
def _e32(seeds, ordinals, shape, slot=0):
    ref = no.noise(seeds, ordinals, shape, slot)
    return ref, float(np.abs(no.noise(seeds, ordinals, shape, slot, np.float32).astype(np.float64) - ref).max())


def test_counter_noise_accuracy():
    from afldm_amd import ops
    shape = (1, 4, 512, 512)                                             # 2^20 values
    ref, e32 = _e32([12345], [3], shape)
    got = ops.counter_noise(_i64([12345]), _i32([3]), shape).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    print(f"[counter noise] seed 12345, ordinal 3, 2^20 values: device max |z - z64| {err:.3e}, numpy float32 E32 {e32:.3e}, "
          f"bound 4 E32 {4 * e32:.3e}")
    assert err <= 4 * e32, (err, e32)
    assert np.abs(got).max() <= 5.77


@pytest.mark.parametrize("shape", [(3, 4, 16, 16), (2, 3, 5, 7)])       # 16-byte stores; scalar, the last group partial
def test_counter_noise_shapes(shape):
    from afldm_amd import ops
    B, n = shape[0], math.prod(shape[1:])
    seeds, ordinals = [5, 1 << 40, 12345][:B], [0, 7, 49][:B]
    ref, e32 = _e32(seeds, ordinals, shape, slot=2)
    got = ops.counter_noise(_i64(seeds), _i32(ordinals), shape, slot=2)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()) <= 4 * e32
    # a base offset by one float: the scalar form, the same bits
    buf = torch.full((B * n + 2,), 9.0, device="cuda")
    off = ops.counter_noise(_i64(seeds), _i32(ordinals), shape, slot=2, out=buf[1:1 + B * n].view(shape))
    assert off.data_ptr() % 16 == 4 and torch.equal(off, got) and float(buf[0]) == 9.0 and float(buf[-1]) == 9.0
    # a sample's values depend on its own seed and ordinal only
    alone = ops.counter_noise(_i64(seeds[1:2]), _i32(ordinals[1:2]), (1,) + shape[1:], slot=2)
    assert torch.equal(alone[0], got[1])


def test_counter_noise_statistics():
    from afldm_amd import ops
    shape = (3, 4, 512, 512)
    z = ops.counter_noise(_i64([0, 1, 12345]), _i32([3, 3, 3]), shape).cpu().numpy().reshape(3, -1)
    for b, seed in enumerate((0, 1, 12345)):
        check_moments(z[b], f"device, seed {seed}, ordinal 3, slot 0, 2^20 values")
    c = ops.counter_noise(_i64([7, 7, 8]), _i32([0, 1, 0]), shape).cpu().numpy().reshape(3, -1)
    s1 = ops.counter_noise(_i64([7]), _i32([0]), (1,) + shape[1:], slot=1).cpu().numpy().reshape(-1)
    check_cross(c[0], c[1], "device, seed 7, ordinal 0 against 1")
    check_cross(c[0], c[2], "device, seed 7 against 8")
    check_cross(c[0], s1, "device, seed 7, slot 0 against 1")


# ------------------------------------------------------------------------------------------------ 3. the seeded step
ROWS = [[1.3, -0.7, -0.9, 1.1, 0.4, 0.8, 0.3, 0.6],                     # an active clamp
        [1.1, -0.5, -math.inf, math.inf, 0.0, 0.9, 0.2, 0.0],           # c = 0: nothing is generated
        [1.2, -0.6, -0.8, 0.7, 0.25, 0.85, 0.35, 0.45],
        [1.05, -0.3, -math.inf, math.inf, 0.0, 0.95, 0.15, 0.3]]
SEEDS = [3, (1 << 62) + 11, 12345]


def _step_inputs(shape, dtype, seed=2):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    eps = torch.randn(B, H, W, C, generator=g).to(dtype)
    return x, eps


def _want(x, eps, z, row):
    """The float32 restatement on the host: x [B, C, H, W], eps NHWC (any dtype), z fp32 NCHW -> the bits as int32."""
    e = eps.float().permute(0, 3, 1, 2).contiguous().numpy()
    return no.update32(x.numpy(), e, z.numpy(), row).view(np.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("plane", [(16, 16), (5, 7)])                   # HW = 256: the 16-byte form; 35: the scalar form
def test_seeded_step_bit_for_bit(plane, dtype):
    from afldm_amd import ops
    shape = (3, 4) + plane
    x, eps = _step_inputs(shape, dtype)
    eps[1, 2, 3, 1] = float("nan")                                       # reaches element (1, 1, 2, 3) of the output alone
    coef = torch.tensor(ROWS, dtype=torch.float64).to(torch.float32)
    xd, ed, cd, sd = x.cuda(), eps.cuda(), coef.cuda().reshape(-1), _i64(SEEDS)
    for k, row in enumerate(ROWS):
        idx = _i32([k])
        z = ops.counter_noise(sd, _i32([k] * 3), shape).cpu() if row[7] != 0.0 else torch.zeros(shape)
        got = ops.seeded_step(xd, ed, sd, cd, idx, advance=(k == 2))
        assert int(idx) == (3 if k == 2 else k), "advance moves the device counter, and only then"
        want, bits = _want(x, eps, z, coef[k].tolist()), _bits(got).numpy()
        nan = np.zeros(shape, dtype=bool)
        nan[1, 1, 2, 3] = True
        assert np.isnan(got.cpu().numpy()[nan]).all() and np.array_equal(bits[~nan], want[~nan]), (k, plane, dtype)
        if k == 0:
            t = coef[0, 0] * x + coef[0, 1] * eps.float().permute(0, 3, 1, 2)
            assert ((t < coef[0, 2]) | (t > coef[0, 3])).any(), "the clamp is active"
    # distinct seeds per sample: sample 0 under sample 2's seed takes sample 2's noise
    idx = _i32([2])
    a = ops.seeded_step(xd, ed, _i64([SEEDS[2], SEEDS[1], SEEDS[0]]), cd, idx)
    z = ops.counter_noise(_i64([SEEDS[2], SEEDS[1], SEEDS[0]]), _i32([2] * 3), shape).cpu()
    want, nan0 = _want(x, eps, z, coef[2].tolist()), np.isnan(a.cpu().numpy())
    assert np.array_equal(_bits(a).numpy()[~nan0], want[~nan0]) and nan0.sum() == 1
    # in place, and the ordinal is the device counter: the same launch with the counter at 3 is row 3 at ordinal 3
    idx = _i32([3])
    inplace = xd.clone()
    assert ops.seeded_step(inplace, ed, sd, cd, idx, out=inplace) is inplace
    z3 = ops.counter_noise(sd, _i32([3] * 3), shape).cpu()
    want3 = _want(x, eps, z3, coef[3].tolist())
    assert np.array_equal(_bits(inplace).numpy()[~nan0], want3[~nan0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("plane", [(16, 16), (5, 7)])
def test_seeded_step_against_sde_step(plane, dtype):
    """afldm_sde_step fed afldm_counter_noise's tensor: the two differ by contraction alone, 8 roundings of at most 2^-24
    relative in each form, so |difference| <= 2^-20 (|a x| + |b| (|p x| + |q e|) + |d e| + |c z|) element by element."""
    from afldm_amd import ops
    shape = (3, 4) + plane
    x, eps = _step_inputs(shape, dtype, seed=9)
    coef = torch.tensor(ROWS, dtype=torch.float64).to(torch.float32)
    xd, ed, cd, sd = x.cuda(), eps.cuda(), coef.cuda().reshape(-1), _i64(SEEDS)
    e = eps.float().permute(0, 3, 1, 2).double()
    for k in (0, 2, 3):
        z = ops.counter_noise(sd, _i32([k] * 3), shape)
        noise = torch.zeros((len(ROWS),) + shape, device="cuda")
        noise[k] = z
        got = ops.seeded_step(xd, ed, sd, cd, _i32([k])).cpu().double()
        ref = ops.sde_step(xd, ed, noise, cd, _i32([k])).cpu().double()
        p, q, lo, hi, a, b, d, c = [abs(float(v)) for v in coef[k]]
        bound = 2.0 ** -20 * (a * x.abs().double() + b * (p * x.abs().double() + q * e.abs()) + d * e.abs() + c * z.cpu().abs().double())
        excess = float(((got - ref).abs() - bound).max())
        print(f"[counter noise] seeded_step against sde_step, row {k}, {plane}, {dtype}: max |difference| "
              f"{float((got - ref).abs().max()):.2e}, max (|difference| - bound) {excess:.2e}")
        assert excess <= 0.0, (k, excess)


def test_rotating_the_batch_rotates_the_result():
    from afldm_amd import ops
    shape = (5, 4, 16, 16)
    x, eps = _step_inputs(shape, torch.bfloat16, seed=4)
    seeds = torch.tensor([3, 1 << 35, 12345, 0, 99], dtype=torch.int64)
    cd = torch.tensor(ROWS, dtype=torch.float64).to(torch.float32).cuda().reshape(-1)
    base = ops.seeded_step(x.cuda(), eps.cuda(), seeds.cuda(), cd, _i32([2]))
    for r in (1, 3):
        rot = ops.seeded_step(x.roll(r, 0).cuda(), eps.roll(r, 0).cuda(), seeds.roll(r, 0).cuda(), cd, _i32([2]))
        assert torch.equal(_bits(rot), _bits(base.roll(r, 0))), r


# ------------------------------------------------------------------------------------------------ 4. the slot step
def _ord(seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 50, (R,), generator=g).to(torch.int32)


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("plane", [5, 16])
@pytest.mark.parametrize("B", [3, 5])
def test_kinds_0_and_1_have_slot_step_kinds_bits(B, plane, dtype, shift):
    """The inputs of tests/test_gpu_slots_dpm.py's step case: x and both history planes are afldm_slot_step_kinds' bit for bit."""
    import slot_oracle as so
    from afldm_amd import ops
    row_coef, row_kind, row_t, row_temb = _tables(3)
    pos, end, state, stretch = _states(B, shift)
    pos, _, active, _ = so.select(row_t, row_temb, pos, end, torch.zeros(B), torch.zeros(T, 4), torch.zeros(B, 4))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 4, plane, plane, generator=g)
    eps = torch.randn(B, plane, plane, 4, generator=g).to(dtype)
    hist = torch.randn(2, B, 4, plane, plane, generator=g)
    xd, ed, hd, cd, kd, pd, ad = (v.cuda() for v in (x, eps, hist, row_coef, row_kind, pos, active))
    want_x, want_h = xd.clone(), hd.clone()
    ops.slot_step_kinds(want_x, ed, want_h, cd, kd, pd, ad)
    got_x, got_h = xd.clone(), hd.clone()
    assert ops.slot_step_seeded(got_x, ed, got_h, cd, kd, _ord().cuda(), pd, ad, _i64(list(range(B)))) is got_x
    assert torch.equal(_bits(got_x), _bits(want_x)) and torch.equal(_bits(got_h), _bits(want_h))
    assert not torch.equal(got_x, xd) and int(active.sum()) >= 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("plane", [5, 16])
def test_a_kind_2_slot_is_seeded_step_and_the_others_are_untouched(plane, dtype):
    """The "ddim" stretch of the table becomes a "seeded" one.  Slots: 0 seeded and active, 1 "dpm" and active, 2 seeded and
    active with a row whose c is 0, 3 inactive, 4 active with pos = R, 5 active with pos = -3, 6 active on a row of code 3."""
    from afldm_amd import ops
    B, C = 7, 4
    row_coef, row_kind, _, _ = _tables(3)
    (d0, d1), (s0, s1) = SPANS[DPM], SPANS[DDIM]
    row_coef[s0:s1] = torch.tensor(ROWS + [ROWS[2]], dtype=torch.float64).to(torch.float32)[:s1 - s0]
    row_kind[s0:s1] = 2
    row_kind[s1 - 1] = 3                                                 # an unknown code
    row_ord = _ord()
    pos = torch.tensor([s0 + 2, d0 + 3, s0 + 1, s0, R, -3, s1 - 1], dtype=torch.int32)
    active = torch.tensor([1, 1, 1, 0, 1, 1, 1], dtype=torch.int32)
    seeds = [41, 42, 43, 44, 45, 46, 47]
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, C, plane, plane, generator=g)
    eps = torch.randn(B, plane, plane, C, generator=g).to(dtype)
    hist = torch.randn(2, B, C, plane, plane, generator=g)
    hist[:, 0, 1] = float("nan")                                         # NaN in a kind-2 slot's history: never read, stays
    for b in (3, 4, 5, 6):
        x[b, 0, 0, 0] = float("nan")
        eps[b] = float("nan")
    xd, ed, hd, cd, kd, od, pd, ad = (v.cuda() for v in (x, eps, hist, row_coef, row_kind, row_ord, pos, active))
    got_x, got_h = xd.clone(), hd.clone()
    ops.slot_step_seeded(got_x, ed, got_h, cd, kd, od, pd, ad, _i64(seeds))
    for b in (0, 2):
        r = int(pos[b])
        k = int(row_ord[r])
        single = torch.zeros(k + 1, 8, device="cuda")
        single[k] = cd[r]
        want = ops.seeded_step(xd[b:b + 1].contiguous(), ed[b:b + 1].contiguous(), _i64(seeds[b:b + 1]), single.reshape(-1), _i32([k]))
        assert torch.equal(_bits(got_x[b:b + 1]), _bits(want)), b
        assert torch.equal(_bits(got_h[:, b]), _bits(hist[:, b])), "a kind-2 slot neither reads nor writes its history"
        assert torch.isfinite(got_x[b]).all()
    assert float(row_coef[int(pos[2]), 7]) == 0.0 and float(row_coef[int(pos[0]), 7]) != 0.0
    # the "dpm" neighbour: afldm_slot_step_kinds' bits
    kinds_x, kinds_h = xd.clone(), hd.clone()
    only = torch.tensor([0, 1, 0, 0, 0, 0, 0], dtype=torch.int32).cuda()
    ops.slot_step_kinds(kinds_x, ed, kinds_h, cd, kd, pd, only)
    assert torch.equal(_bits(got_x[1]), _bits(kinds_x[1])) and torch.equal(_bits(got_h[:, 1]), _bits(kinds_h[:, 1]))
    assert not torch.equal(got_h[:, 1], hd[:, 1])
    for b in (3, 4, 5, 6):
        assert torch.equal(_bits(got_x[b]), _bits(x[b])) and torch.equal(_bits(got_h[:, b]), _bits(hist[:, b])), b
    assert torch.equal(pd.cpu(), pos) and torch.equal(ad.cpu(), active)
