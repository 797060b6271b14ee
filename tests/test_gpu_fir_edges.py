"""afldm_upfirdn2d (csrc/fir.hip) on MI355X at every class of launch that plumbing_oracle.fir_route tells apart: the
vec, slide and general column routes (and the launch that mixes the first two), both row templates, a second and a third
x block, the plane loop past 4096 planes, the second pass of the tap copy and the 64 KiB tap limit.  Inputs are small
integers and taps multiples of 1/8, so that every partial sum is exact in fp32 in any order: the output must EQUAL the
float64 reference (oracle.upfirdn.upfirdn2d on a float64 x), in bf16 its round-to-nearest-even rounding.  One case with
real-valued data is held to a per-element bound.  Derivations: the docstring of tests/plumbing_oracle.py.

Measured on one MI355X: this file (95 tests) and tests/test_gpu_plumbing.py (94 tests) together run in 2.7 s of
pytest time in one process; no single test takes 0.5 s."""
import pytest
import torch

import plumbing_oracle as po

pytestmark = pytest.mark.gpu
DTYPES = list(po.DTYPES)
IDS = ["fp32", "bf16"]
BY_NAME = {c["name"]: c for c in po.FIR_CASES}
_REF = {}


def _ops():
    from afldm_amd import ops
    return ops


def _case_data(c):
    """(x, f, float64 reference) of a case, computed once and shared."""
    if c["name"] not in _REF:
        x, f = po.fir_inputs(c)
        _REF[c["name"]] = (x, f, po.fir_reference(c, x, f))
    return _REF[c["name"]]


def _device_input(c, x, dtype):
    """x on the device; for an `offset` case a contiguous view that starts one element past a 16-byte boundary."""
    x = x.to(dtype)
    if not c["offset"]:
        xd = x.cuda()
        assert xd.data_ptr() % 16 == 0
        return xd
    buf = torch.zeros(x.numel() + 8, dtype=dtype, device="cuda")
    xd = buf[1:1 + x.numel()].view(x.shape)
    xd.copy_(x)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == x.element_size()
    return xd


def _launch(c, xd, f2, out=None):
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = c["up"], c["down"], c["pad"]
    return _ops().upfirdn2d(xd, f2.cuda(), ux, uy, dx, dy, px0, px1, py0, py1, c["flip"], c["gain"], out=out)


def _same(got, want, c, what):
    outH, outW = po.fir_out_size(c)
    po.assert_identical(got.reshape(-1, outH, outW), want.reshape(-1, outH, outW), f"{c['name']} {what}",
                        names=("plane", "oy", "ox"), extra=str(po.fir_route(c)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", po.FIR_CASES, ids=lambda c: c["name"])
def test_every_route_exact(case, dtype):
    c = case
    x, f, ref = _case_data(c)
    want = ref.float().to(dtype)                                              # ref is an fp32 value (host test): one rounding
    xd = _device_input(c, x, dtype)
    got = _launch(c, xd, po.fir_filter_2d(c, f))
    assert got.dtype == dtype and got.shape == want.shape
    _same(got, want, c, "2-D launch")
    if c["f1d"]:                                                              # the two-pass separable form
        from afldm_amd.af_libs.torch_utils.ops import upfirdn2d as up
        sep = up.upfirdn2d(xd, f.cuda(), **po.fir_kwargs(c))
        two = want if dtype == torch.float32 else po.fir_reference_two_pass(c, x, f, dtype).float().to(dtype)
        _same(sep, two, c, "separable")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["vec_padx1", "slide_fw7_padx0_2", "general_x32_y21", "slide_w257"])
def test_out_form_keeps_canaries_and_repeats(name, dtype):
    c = BY_NAME[name]
    x, f, ref = _case_data(c)
    want = ref.float().to(dtype)
    xd, f2 = _device_input(c, x, dtype), po.fir_filter_2d(c, f)
    buf, view = po.with_canaries(tuple(want.shape), dtype, "cuda")
    assert _launch(c, xd, f2, out=view).data_ptr() == view.data_ptr()
    _same(view, want, c, "out=")
    assert po.canaries_intact(buf, want.numel())
    again = _launch(c, xd, f2)
    po.assert_identical(again, view, f"{name} repeat call", by_bits=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_planes_are_independent(dtype):
    c = BY_NAME["planes_4097"]
    x, f, _ = _case_data(c)
    full = _launch(c, x.to(dtype).cuda(), f)
    for p in (0, 4095, 4096):
        one = _launch(dict(c, planes=(1, 1)), x[p:p + 1].clone().to(dtype).cuda(), f)
        po.assert_identical(full[p:p + 1], one, f"plane {p} of the 4097-plane launch", by_bits=True, names=("b", "c", "oy", "ox"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_real_valued_lanczos(dtype):
    from oracle import upfirdn as ou
    from afldm_amd.af_libs.torch_utils.ops import upfirdn2d as up
    x, f = po.real_fir_case()
    x = x.to(dtype)
    f2 = torch.outer(f, f)
    pad = (6, 6, 6, 6)
    ref = ou.upfirdn2d(x.double(), f2, padding=list(pad))
    tol = po.real_fir_tolerance(x, f2, ref, pad, dtype)
    got = _ops().upfirdn2d(x.cuda(), f2.cuda(), 1, 1, 1, 1, *pad)
    assert got.dtype == dtype
    po.assert_within(got.cpu(), ref, tol, f"13-tap Lanczos, 2-D, {dtype}")
    if dtype == torch.float32:                                                # two passes round less often than 13 x 13 taps
        sep = up.upfirdn2d(x.cuda(), f.cuda(), padding=list(pad))
        po.assert_within(sep.cpu(), ref, tol, "13-tap Lanczos, separable, fp32")


def test_tap_buffer_limit():
    """128 x 128 taps (64 KiB) launch (FIR_CASES holds the value test); one tap row more is refused before any launch."""
    from afldm_amd import _lib as L
    assert po.fir_route(BY_NAME["taps_128x128"]).tap_loop
    r = po.FIR_REFUSED
    x = torch.zeros(r["H"] * r["W"], device="cuda")
    f = torch.ones(r["fh"] * r["fw"], device="cuda")
    y = torch.full((64,), -77.0, device="cuda")
    rc = L.lib.afldm_upfirdn2d(x.data_ptr(), f.data_ptr(), y.data_ptr(), r["planes"], r["H"], r["W"], r["fh"], r["fw"],
                               1, 1, 1, 1, 0, 0, 0, 0, 0, 1.0, L.F32, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.ABI.constants["AFLDM_ESHAPE"] and b"64 KiB" in L.lib.afldm_last_error()
    assert bool((y == -77.0).all())
