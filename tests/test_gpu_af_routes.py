"""Every route of the alias-free activation (afldm_af_act) and of the small resampling sites (afldm_af_resample), at shapes
of a few hundred KB, against the float64 oracle.

Which kernel a call runs is decided on the host (af_act_plan / resample_plan in csrc/af.hip) from the batch, the byte count
and the CU count; at the B = 2 / 3 shapes of the other test files most of the choices the benchmark makes are never taken.
Here the choice is forced with ops.af_tune, `max_grid` makes a tensor of a few items give several items per workgroup (the
first item of a workgroup finishes its GroupNorm statistics in line, the later ones are pipelined where the instantiation
has that path), and every comparison first asserts through ops.af_act_route that the route it is meant for is the one taken.

Reference: float64 GroupNorm from the same hand-made partial sums the kernel is given (test_gpu_groupnorm_stats.Case: every
(sample, group) has its own mean and deviation, every channel its own gamma / beta, so a wrong sample, group or channel index
moves values by O(1)), then oracle.ideal_filters.warped_nonlinearity in float64.

Tolerance: the classes of test_gpu_ops.close (fp32: max error <= 2e-5 max|ref|; bf16: rel-RMS <= 1e-2, max <= 8e-2), applied
to the whole tensor and, with the same number, to every (sample, channel) plane:
    RMS(plane error) <= class tolerance x max(RMS(plane reference), RMS(whole reference))
so that one wrong plane cannot hide in the mean over the tensor.  Each check prints its worst plane as a fraction of that.

COVERED is the set of routes (dtype, N, kernel, channels per item, several items per workgroup) compared here with the
reference; tests/test_af_routes_host.py asserts that every activation site of the FFHQ AF-UNet plans into it at every
benchmark batch size."""
import functools

import pytest
import torch

from test_gpu_groupnorm_stats import AF_SHAPES, Case, _warped
from test_gpu_ops import close

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
RATIO, STARVE, CONST = 8, False, 0.25          # the hard planes of gn_oracle at |mean| / std up to 8
CLASS_TOL = {F32: 2e-5, BF16: 1e-2}


def _ops():
    from afldm_amd import ops
    return ops


def _id(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, (tuple, list)):
        return "-".join(str(i) for i in v)
    return str(v)


def route_key(dtype, N, route):
    return (_id(dtype), N, route.kernel, route.ch, route.kernel == "plane" and route.items_per_wg > 1)


def close_planes(got, ref, dtype, what, bf16_rms=1e-2):
    """close() over the tensor, then its class tolerance per (sample, channel) plane of got / ref [B, N, N, C]."""
    close(got, ref, dtype, what, bf16_rms=bf16_rms)
    got, ref = got.double(), ref.double()
    tol = CLASS_TOL[F32] if dtype == F32 else bf16_rms
    err = (got - ref).pow(2).mean((1, 2)).sqrt()
    scale = torch.maximum(ref.pow(2).mean((1, 2)).sqrt(), ref.pow(2).mean().sqrt())
    frac = (err / scale / tol).max().item()
    b, c = divmod(int((err / scale).argmax()), err.shape[1])
    print(f"[{what}] worst plane (b={b}, c={c}): RMS error / (tol x scale) = {frac:.3f}")
    assert frac <= 1.0, f"{what}: plane (b={b}, c={c}) off by {frac:.2f} x the per-plane tolerance {tol}"
    return frac


@functools.lru_cache(maxsize=None)
def _case(B, N, C1, C2, G, dtype, S1, S2):
    """(Case, float64 reference [B, N, N, C]) - built once per shape and shared; nobody writes to either."""
    case = Case(B, C1, C2, G, N * N, dtype, RATIO, STARVE, CONST, S1, S2, seed=N + C1)
    return case, _warped(case.ref, B, N, C1 + C2)


def _act(case, N, expect, tune, **kw):
    """af_act under `tune`, after asserting that the planner reports `expect` = (kernel, ch[, grid, items per workgroup])."""
    ops = _ops()
    x1, x2, stats, gamma, beta = case.dev((N, N))
    if kw.pop("x_c8", False):
        from test_gpu_r05 import _nhwc_to_c8
        x1 = _nhwc_to_c8(x1)
    with ops.af_tune(**tune):
        r = ops.af_act_route(case.dtype, N, case.C1, case.C2, case.B)
        assert tuple(r)[:len(expect)] == tuple(expect), f"planned {r}, the case is meant for {expect} (tune {tune})"
        assert route_key(case.dtype, N, r) in COVERED, r
        return ops.af_act(x1, x2, stats, gamma, beta, case.G, case.eps, **kw)


# ------------------------------------------------------------------------------------------------ default routes
def _default_route(dtype, N, C1, C2):
    """What the planner picks for the B = 3 rows of AF_SHAPES with nothing forced, on 256 CUs."""
    c16 = C1 % 16 == 0 and C2 % 16 == 0
    if N >= 16:
        return ("plane", 8)
    if N == 8 and c16:
        return ("p8", 0) if dtype == BF16 else ("kron", 0)
    return ("small", 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", AF_SHAPES, ids=_id)
def test_default_routes_per_plane(shape, dtype):
    """The routes the other files already compare over the whole tensor, here also plane by plane (B = 3, nothing forced)."""
    N, C1, C2, G = shape
    case, ref = _case(3, N, C1, C2, G, dtype, 9, 4 if C2 else 0)
    y = _act(case, N, _default_route(dtype, N, C1, C2), {})
    close_planes(y.float().cpu(), ref, dtype, f"af_act default {shape}")


# ------------------------------------------------------------------------------------------------ a. plane kernel
PLANE_SHAPES = [
    # C1, C2, G
    (32, 0, 8),              # cpg = 4
    (16, 32, 8),             # cpg = 6: seam inside group 2, items lying wholly in x2
    (64, 0, 64),             # cpg = 1: an item touches 8 / 16 groups (> 4 waves), so `fast` / `n_piped` are off
    (48, 0, 2),              # cpg = 24: in line at S = 9 (24 * 9 > 128 partials), pipelined at S = 1
]
PLANE_INST = [(d, N, CH) for d in DTYPES for N in (16, 32) for CH in (8, 16)]


def _plane_splits(C2):
    return [(1, 32), (9, 4)] if C2 else [(1, 0), (9, 0)]


def _plane_expect(C, CH, max_grid, B=2):
    items = B * (C // CH)
    grid = min(items, max_grid) if max_grid else items
    return ("plane", CH, grid, -(-items // grid))


@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=_id)
@pytest.mark.parametrize("dtype,N,CH", PLANE_INST, ids=_id)
def test_plane_kernel_several_items_per_workgroup(dtype, N, CH, shape):
    """k_af_act_plane<T, N, CH> with two workgroups of 2 - 8 items each (one sample per workgroup): the first item (statistics in
    line or with the second one's), the middle ones (pipelined in <16, 8> and <32, 16>) and the last, every element."""
    C1, C2, G = shape
    for S1, S2 in _plane_splits(C2):
        case, ref = _case(2, N, C1, C2, G, dtype, S1, S2)
        expect = _plane_expect(C1 + C2, CH, 2)
        assert expect[3] >= 2
        y = _act(case, N, expect, dict(ch=CH, max_grid=2))
        close_planes(y.float().cpu(), ref, dtype, f"plane<{_id(dtype)}, {N}, {CH}> {shape} S=({S1},{S2}) grid 2")


@pytest.mark.parametrize("max_grid", [1, 0], ids=["one-workgroup", "no-cap"])
@pytest.mark.parametrize("dtype,N,CH", PLANE_INST, ids=_id)
def test_plane_kernel_one_workgroup_and_one_item_each(dtype, N, CH, max_grid):
    """All items in one workgroup (it crosses from sample 0 to sample 1), and one item per workgroup (no cap)."""
    C1, C2, G = PLANE_SHAPES[1]
    case, ref = _case(2, N, C1, C2, G, dtype, 9, 4)
    y = _act(case, N, _plane_expect(C1 + C2, CH, max_grid), dict(ch=CH, max_grid=max_grid))
    close_planes(y.float().cpu(), ref, dtype, f"plane<{_id(dtype)}, {N}, {CH}> max_grid={max_grid}")


# ------------------------------------------------------------------------------------------------ b. layouts
@pytest.mark.parametrize("N,CH", [(16, 8), (16, 16), (32, 8), (32, 16)], ids=_id)
def test_plane_kernel_c8_layouts_on_both_item_sizes(N, CH):
    """8-channel blocks in and / or out (bf16): with CH = 16 a pixel of an item spans two blocks.  Bit for bit the NHWC result of
    the same route, which test_plane_kernel_several_items_per_workgroup compares with the reference."""
    from test_gpu_r05 import _c8_to_nhwc
    ops = _ops()
    tune = dict(ch=CH, max_grid=2)
    for C1, C2, G in PLANE_SHAPES:
        for S1, S2 in _plane_splits(C2)[1:]:
            case, _ = _case(2, N, C1, C2, G, BF16, S1, S2)
            expect = _plane_expect(C1 + C2, CH, 2)
            what = f"plane<bf16, {N}, {CH}> {(C1, C2, G)}"
            y = _act(case, N, expect, tune)
            y8 = _act(case, N, expect, tune, out_c8=True)
            assert ops.is_c8(y8) and torch.equal(_c8_to_nhwc(y8), y), what + ": NHWC -> c8"
            if not C2:                                         # a blocked input is a single tensor
                y88 = _act(case, N, expect, tune, x_c8=True, out_c8=True)
                assert ops.is_c8(y88) and torch.equal(_c8_to_nhwc(y88), y), what + ": c8 -> c8"
                y80 = _act(case, N, expect, tune, x_c8=True)
                assert not ops.is_c8(y80) and torch.equal(y80, y), what + ": c8 -> NHWC"


# ------------------------------------------------------------------------------------------------ c. cross-route agreement
@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=_id)
@pytest.mark.parametrize("N", [16, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_plane_kernel_item_size_does_not_change_a_bit(dtype, N, shape):
    """CH decides which wave owns which plane, how the tile is staged and which of the three statistics paths an item takes
    (PlaneCfg: CPW = CH / 4, XS, YRP); inside a plane the four passes of af_plane_passes.inc run the same MFMA chains in the
    same order, and the statistics paths add the same terms in the same order.  So the two item sizes agree bit for bit."""
    C1, C2, G = shape
    for S1, S2 in _plane_splits(C2):
        case, _ = _case(2, N, C1, C2, G, dtype, S1, S2)
        y8, y16 = (_act(case, N, _plane_expect(C1 + C2, CH, 2), dict(ch=CH, max_grid=2)) for CH in (8, 16))
        assert torch.equal(y8, y16), f"{_id(dtype)} N={N} {shape} S=({S1},{S2}): CH = 8 and CH = 16 differ"


# ------------------------------------------------------------------------------------------------ f. stagger
@pytest.mark.parametrize("dtype,N,CH", [(BF16, 16, 8), (F32, 32, 16)], ids=_id)
def test_plane_kernel_stagger_only_delays(dtype, N, CH):
    C1, C2, G = PLANE_SHAPES[1]
    case, _ = _case(2, N, C1, C2, G, dtype, 9, 4)
    expect = _plane_expect(C1 + C2, CH, 2)
    y0 = _act(case, N, expect, dict(ch=CH, max_grid=2, stagger=0))
    y1 = _act(case, N, expect, dict(ch=CH, max_grid=2, stagger=1))
    assert torch.equal(y0, y1)


# ------------------------------------------------------------------------------------------------ d. small planes
def _rows(N, also=()):
    return [(3,) + s for s in AF_SHAPES if s[0] == N] + list(also)


RAGGED = lambda N: (5, N, 16, 0, 4)             # 5 items: the second group of four (kron) / tile of four (p8) holds one
SMALL_CASES = (
    # kernel forced, dtypes, tune, rows (B, N, C1, C2, G)
    [("kron", DTYPES, dict(small_n=0), _rows(4, [RAGGED(4)])),
     ("kron", [BF16], dict(p8=0), _rows(8, [RAGGED(8)])),
     ("kron", [F32], dict(), _rows(8, [RAGGED(8)])),
     ("small", DTYPES, dict(), _rows(4)),
     ("small", DTYPES, dict(small_n=12), _rows(8, [(3, 8, 24, 12, 6)])),      # the last: C % 16 != 0 with GroupNorm at N = 8
     ("small", DTYPES, dict(), [(3, 8, 24, 12, 6)]),                          # ... which is the VALU kernel by default too
     ("p8", [BF16], dict(), _rows(8, [RAGGED(8)]))])
SMALL_PARAMS = [(k, d, tuple(sorted(t.items())), row) for k, ds, t, rows in SMALL_CASES for d in ds for row in rows]


@pytest.mark.parametrize("kernel,dtype,tune,row", SMALL_PARAMS, ids=_id)
def test_small_plane_kernels(kernel, dtype, tune, row):
    """k_af_act_kron<T, 4 / 8>, k_af_act_small<T, 4 / 8> and k_af_act_p8 each on the N = 4 / 8 rows of AF_SHAPES; a row whose
    channel counts are no multiples of 16 is the VALU kernel's whatever is forced."""
    B, N, C1, C2, G = row
    if C1 % 16 or C2 % 16:
        kernel = "small"
    case, ref = _case(B, N, C1, C2, G, dtype, 9, 4 if C2 else 0)
    y = _act(case, N, (kernel, 0), dict(tune))
    close_planes(y.float().cpu(), ref, dtype, f"{kernel}<{_id(dtype)}, {N}> {row} tune={dict(tune)}")


# ------------------------------------------------------------------------------------------------ the routes compared above
COVERED = (
    {(_id(d), s[0]) + _default_route(d, *s[:3]) + (False,) for d in DTYPES for s in AF_SHAPES}
    | {(_id(d), N, "plane", CH, several) for d, N, CH in PLANE_INST for several in (False, True)}
    | {(_id(d), row[1], k if not (row[2] % 16 or row[3] % 16) else "small", 0, False) for k, d, _, row in SMALL_PARAMS})


# (N, C1, C2) of every distinct ops.af_act call of the FFHQ AF-UNet; tests/test_af_routes_host.py plans each of them at the
# benchmark batch sizes.  The test below keeps the table equal to what the model does.
FFHQ_AF_ACT_SITES = [
    (2, 768, 0), (2, 768, 768), (4, 384, 0), (4, 768, 0), (4, 768, 384), (4, 768, 768), (8, 384, 0), (8, 384, 384), (8, 768, 384),
    (16, 192, 0), (16, 384, 0), (16, 384, 192), (16, 384, 384), (32, 192, 0), (32, 192, 192), (32, 384, 192)]


def test_ffhq_unet_activation_sites_are_the_table(monkeypatch):
    from test_gpu_r02 import build_unet
    ops = _ops()
    unet, _, _ = build_unet("ffhq", BF16)
    seen, real = set(), ops.af_act

    def record(x1, x2=None, *a, **k):
        seen.add((x1.shape[1], x1.shape[-1], 0 if x2 is None else x2.shape[-1]))
        return real(x1, x2, *a, **k)
    monkeypatch.setattr(ops, "af_act", record)
    unet(torch.zeros(2, 4, 32, 32, device="cuda", dtype=BF16), 501, return_dict=False)
    assert sorted(seen) == FFHQ_AF_ACT_SITES


# ------------------------------------------------------------------------------------------------ e. resampling
RESAMPLE_SITES = [(2, 4, 1), (4, 8, 1), (8, 16, 1), (8, 16, 2), (8, 16, 4), (4, 2, 1), (8, 4, 1)]      # N, R, SPLIT


@pytest.mark.parametrize("C", [4, 64, 100])      # 12 planes: the ragged tail of a 256-thread workgroup; C % 16 != 0
@pytest.mark.parametrize("N,R,split", RESAMPLE_SITES, ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_small_resampling_sites_one_launch_against_two_passes(dtype, N, R, split, C):
    """k_resample_small<T, N, R, SPLIT> against the two register-blocked passes (k_axis_contract_reg) that csrc/af.hip says it
    equals bit for bit, values and emitted GroupNorm partial sums, and both against the oracle's rfft definition in float64, in the
    class test_af_resample uses (bf16 rel-RMS 4e-3).  Per plane that number is met by construction, not by luck of the seed: the
    fp32 chains are good to ~1e-6 and the one rounding of the stored value is at most 2^-8 |v| = 3.9e-3 |v| element by element,
    so a plane's RMS error stays below 0.98 of the tolerance however few pixels it has (measured: up to 0.95 on the 2 x 2 outputs)."""
    from oracle import ideal_filters as idf
    from test_gpu_ops import back, nhwc, rnd
    ops = _ops()
    B = 3
    x = rnd(dtype, torch.randn(B, C, N, N, generator=torch.Generator().manual_seed(100 * N + C)))
    xh = nhwc(x, dtype)
    up = R == 2 * N
    ref = idf.upsample_rfft(x.double(), 2) if up else idf.lpf_rfft(x.double())[:, :, ::2, ::2]
    run = (lambda: ops.af_up2(xh)) if up else (lambda: ops.af_lpf_down2(xh, want_stats=True))
    with ops.af_tune(resample_split=split):
        assert ops.af_resample_route(N, C, R) == ("small", split)
        one = run()
    with ops.af_tune(no_resample_small=1):
        assert ops.af_resample_route(N, C, R) == ("reg", 0)
        two = run()
    assert ops.af_resample_route(N, C, R) == ("small", 4 if (N, R) == (8, 16) else 1)       # the defaults are back
    what = f"resample {N}->{R} split={split} C={C}"
    assert one.shape == (B, R, R, C) and torch.equal(one, two), what + ": one launch and two passes differ"
    if not up:
        assert one.gn_partial.shape == (B, R, C, 2) and torch.equal(one.gn_partial, two.gn_partial), what + ": statistics differ"
    close_planes(back(one).permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1), dtype, what, bf16_rms=4e-3)


def test_af_tune_refuses_bad_values_and_resets():
    ops = _ops()
    for bad in (dict(ch=4), dict(small_n=3), dict(resample_split=3), dict(max_grid=-1), dict(stagger=-1)):
        with pytest.raises(RuntimeError, match="afldm_af_tune"):
            with ops.af_tune(**bad):
                pass
    with pytest.raises(TypeError):
        with ops.af_tune(chh=8):
            pass
    before = ops.af_act_route(BF16, 32, 64, 0, 2, cus=256)
    with ops.af_tune(ch=16, max_grid=1):
        assert ops.af_act_route(BF16, 32, 64, 0, 2, cus=256) == ("plane", 16, 1, 8)
    assert ops.af_act_route(BF16, 32, 64, 0, 2, cus=256) == before == ("plane", 8, 16, 1)
