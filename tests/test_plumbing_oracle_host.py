"""CPU proof of tests/plumbing_oracle.py: the float64 FIR reference equals the operator spelt out as a loop, the FIR
case list reaches every class of launch that fir_route tells apart, the tolerances dominate the error counts they are
derived from, and every planted fault fails the comparison the GPU files use, with the element named."""
import math

import pytest
import torch

import plumbing_oracle as po

BY_NAME = {c["name"]: c for c in po.FIR_CASES}


# ------------------------------------------------------------------------------------------------ FIR reference
@pytest.mark.parametrize("case", po.FIR_CASES, ids=lambda c: c["name"])
def test_fir_reference_equals_the_loop(case):
    x, f = po.fir_inputs(case)
    assert po.fir_exact(case, f), "a partial sum of this case could round in fp32"
    assert float(x.abs().max()) <= 8 and bool((x == x.round()).all())
    ref = po.fir_reference(case, x, f)
    assert ref.dtype == torch.float64 and tuple(ref.shape[2:]) == po.fir_out_size(case)
    po.assert_identical(ref, po.fir_loop(case, x, po.fir_filter_2d(case, f)), case["name"], names=po.fir_names())
    assert bool((ref.float().double() == ref).all())                       # the expected output is an fp32 value
    if case["f1d"]:                                                        # two exact fp32 passes give the same value
        po.assert_identical(po.fir_reference_two_pass(case, x, f, torch.float32), ref, case["name"] + " two-pass")


def test_fir_loop_flips_and_negative_pads():
    """Both flips and a crop on each side go through the comparison above; here the flag itself is shown to matter."""
    flips = {c["flip"] for c in po.FIR_CASES}
    assert flips == {False, True}
    for side in range(4):
        assert any(c["pad"][side] < 0 for c in po.FIR_CASES), side
    c = BY_NAME["general_x32_y21"]
    x, f = po.fir_inputs(c)
    assert not torch.equal(po.fir_loop(c, x, f), po.fir_loop(c, x, f, flip=not c["flip"]))


def test_fir_cases_cover_every_class():
    R = {c["name"]: po.fir_route(c) for c in po.FIR_CASES}
    routes = set(R.values())
    have = lambda pred: any(pred(BY_NAME[n], r) for n, r in R.items())          # noqa: E731
    assert have(lambda c, r: r.route == "vec" and r.last_group == "vec")
    assert have(lambda c, r: r.route == "vec" and r.last_group == "slide" and c["pad"][1] > 0)      # the mixed launch
    assert have(lambda c, r: r.route == "slide" and c["fw"] == 1 and c["W"] % 4 != 0)
    assert have(lambda c, r: r.route == "slide" and c["fw"] == 1 and c["offset"] and c["W"] % 4 == 0)
    for fw in (2, 7):
        for sign in (-1, 0, 1):
            assert have(lambda c, r: r.route == "slide" and c["fw"] == fw and (c["pad"][0] > 0) - (c["pad"][0] < 0) == sign), (fw, sign)
    assert have(lambda c, r: r.route == "slide" and c["fw"] > c["W"])
    for ratio in ((2, 1), (1, 2), (3, 2)):
        assert have(lambda c, r: r.route == "general" and (c["up"][0], c["down"][0]) == ratio), ratio
        assert have(lambda c, r: (c["up"][1], c["down"][1]) == ratio and (c["up"][0], c["down"][0]) != ratio), ratio
    for side in range(4):
        assert have(lambda c, r: r.route == "general" and c["pad"][side] < 0), side
    for route in ("vec", "slide", "general"):
        for outW, blocks in ((255, 1), (256, 1), (257, 2), (513, 3)):
            assert have(lambda c, r: r.route == route and po.fir_out_size(c)[1] == outW and r.x_blocks == blocks), (route, outW)
        for RY in (1, 4):
            assert have(lambda c, r: r.route == route and r.RY == RY and r.x_blocks > 1), (route, RY)
    assert have(lambda c, r: r.route == "slide" and c["fw"] > 1 and r.RY == 4)
    for outH, RY in ((1, 1), (15, 1), (16, 4), (17, 4)):
        assert have(lambda c, r: po.fir_out_size(c)[0] == outH and r.RY == RY), outH
    assert have(lambda c, r: r.plane_loop and c["planes"][0] * c["planes"][1] == 4097 and (c["H"], c["W"], c["fh"], c["fw"]) == (4, 4, 1, 1))
    assert have(lambda c, r: r.tap_loop and (c["fh"], c["fw"]) == (17, 16))
    assert have(lambda c, r: (c["fh"], c["fw"], c["H"], c["W"]) == (128, 128, 128, 128))
    assert 4 * 128 * 128 == po.FIR_MAX_TAP_BYTES and 4 * po.FIR_REFUSED["fh"] * po.FIR_REFUSED["fw"] > po.FIR_MAX_TAP_BYTES
    assert {c["gain"] for c in po.FIR_CASES} == {1.0, 0.5, 4.0}
    assert {c["flip"] for c in po.FIR_CASES} == {False, True}
    assert have(lambda c, r: c["f1d"] and r.route == "slide") and have(lambda c, r: c["f1d"] and r.route == "general")
    assert {r.route for r in routes} == {"vec", "slide", "general"}
    assert max(c["planes"][0] * c["planes"][1] * c["H"] * c["W"] for c in po.FIR_CASES) <= 1_100_000
    # losing a class is noticed: the list without its mixed launches fails the first guard
    rest = [r for n, r in R.items() if not (r.route == "vec" and r.last_group == "slide")]
    assert not any(r.route == "vec" and r.last_group == "slide" for r in rest) and len(rest) < len(R)


def test_fir_route_follows_the_launch_conditions():
    c = po.fir_case("t", (1, 1), 8, 8, fh=3, fw=1, pad=(0, 0, 1, 1))
    assert po.fir_route(c) == po.FirRoute("vec", "vec", 1, 1, False, False)
    assert po.fir_route(dict(c, pad=(0, 1, 1, 1))).last_group == "slide"
    assert po.fir_route(dict(c, pad=(0, -1, 1, 1))) == po.FirRoute("vec", "vec", 1, 1, False, False)   # 7 columns: the group still fits W
    assert po.fir_route(dict(c, pad=(1, 0, 1, 1))).route == "slide"
    assert po.fir_route(dict(c, offset=True)).route == "slide"
    assert po.fir_route(dict(c, W=9)).route == "slide"
    assert po.fir_route(dict(c, fw=2, pad=(1, 0, 1, 1))).route == "slide"
    assert po.fir_route(dict(c, up=(2, 1))).route == "general" and po.fir_route(dict(c, down=(2, 1))).route == "general"
    assert po.fir_route(dict(c, up=(1, 2))).route == "vec"                      # y re-sampling does not choose the route
    assert po.fir_route(dict(c, H=16)).RY == 4 and po.fir_route(dict(c, H=15)).RY == 1
    assert po.fir_route(dict(c, W=260)).x_blocks == 2
    assert po.fir_route(dict(c, planes=(64, 64))).plane_loop is False and po.fir_route(dict(c, planes=(4097, 1))).plane_loop
    assert po.fir_route(dict(c, H=40, fh=16, fw=16, W=40)).tap_loop is False and po.fir_route(dict(c, H=40, fh=17, fw=16, W=40)).tap_loop


# ------------------------------------------------------------------------------------------------ planted faults
def _fails(got, want, needle, **kw):
    with pytest.raises(AssertionError) as e:
        po.assert_identical(got, want, "planted", **kw)
    assert needle in str(e.value), str(e.value)
    return str(e.value)


def _first_unequal_neighbours(t):
    flat = t.reshape(-1)
    return int(torch.nonzero(flat[1:] != flat[:-1])[0])


def _planted(ref):
    """(name, faulty copy, flat index of the first wrong element) for a [B, C, H, W] result with more than one plane."""
    B, C, H, W = ref.shape
    out = []
    k = _first_unequal_neighbours(ref)
    sw = ref.clone().reshape(-1)
    sw[k], sw[k + 1] = ref.reshape(-1)[k + 1], ref.reshape(-1)[k]
    out.append(("swapped neighbours", sw.reshape(ref.shape), k))
    planes = ref.reshape(B * C, H, W)
    p = next(i for i in range(B * C - 1) if not torch.equal(planes[i, -1], planes[i + 1, -1]))
    row = planes.clone()
    row[p, -1] = planes[p + 1, -1]
    first = int(torch.nonzero(row[p, -1] != planes[p, -1])[0])
    out.append(("last row from the next plane", row.reshape(ref.shape), (p * H + H - 1) * W + first))
    grp = planes.clone()
    g0 = next(g for g in range(0, W - 4, 4) if not torch.equal(planes[0, 0, g:g + 4], planes[0, 0, g + 1:g + 5]))
    grp[0, 0, g0:g0 + 4] = planes[0, 0, g0 + 1:g0 + 5]
    first = int(torch.nonzero(grp[0, 0] != planes[0, 0])[0])
    out.append(("column group shifted by one", grp.reshape(ref.shape), first))
    return out


@pytest.mark.parametrize("name", ["slide_fw7_padx0_2", "general_x32_y21", "vec_padx1"])
def test_planted_fir_faults_are_caught_and_named(name):
    c = BY_NAME[name]
    x, f = po.fir_inputs(c)
    ref = po.fir_reference(c, x, f).float()
    for what, bad, flat in _planted(ref):
        _fails(bad, ref, f"first at flat {flat} ", names=po.fir_names())
    f2 = po.fir_filter_2d(c, f)
    if c["fh"] > 1:
        dropped = po.fir_loop(c, x, f2, drop_tap_row=c["fh"] - 1).float()
        msg = _fails(dropped, ref, "oy=", names=po.fir_names())
        assert "ox=" in msg and "b=" in msg
    if c["fh"] * c["fw"] > 1:
        _fails(po.fir_loop(c, x, f2, flip=not c["flip"]).float(), ref, "oy=", names=po.fir_names())


def test_planted_truncation_is_caught():
    """bf16 by truncation differs from RNE on the rounding probes and on a FIR output that is not a bf16 value."""
    p = po.rounding_probes()
    want = po.expected_bf16(p)
    _fails(po.truncate_bf16(p), want, "first at flat 1 ", by_bits=True)        # the tie above an odd mantissa rounds up
    assert math.isinf(float(want[7])) and float(want[7]) > 0                   # the largest finite fp32 rounds to +inf
    assert po.bits(want)[0] == 0x3F80 and po.bits(want)[1] == 0x3F82 and po.bits(want)[2] == 0x3F81
    assert bool(torch.isnan(want[22])) and po.bits(want)[13] == -32768          # NaN stays NaN, -0 keeps its sign
    c = BY_NAME["slide_fw7_padx0_2"]
    x, f = po.fir_inputs(c)
    ref = po.fir_reference(c, x, f).float()
    assert not torch.equal(ref.to(torch.bfloat16).float(), ref)
    _fails(po.truncate_bf16(ref), ref.to(torch.bfloat16), "oy=", names=po.fir_names())


@pytest.mark.parametrize("dtype", po.DTYPES)
def test_planted_layout_faults_are_caught_and_named(dtype):
    B, C, H, W = 2, 3, 5, 7
    x = po.addressed(B * C * H * W, dtype).reshape(B, C, H, W)
    want = po.nhwc_reference(x).permute(0, 3, 1, 2)          # any 4-D view does: the faults are defined on [.., H, W]
    want = want.contiguous()
    for what, bad, flat in _planted(want):
        msg = _fails(bad, want, f"first at flat {flat} ", by_bits=True)
        if dtype == torch.float32:                           # the message holds the source indices fetched and wanted
            assert f"want {float(want.reshape(-1)[flat])!r}" in msg and f"got {float(bad.reshape(-1)[flat])!r}" in msg
    # a transposition that is not done at all, and one done with the wrong stride
    _fails(x.reshape(B, H, W, C), po.nhwc_reference(x), "first at flat 1 ", by_bits=True)
    w = po.addressed(4 * 6 * 3, dtype).reshape(4, 6, 1, 3)
    _fails(w.reshape(4, 1, 3, 6), po.pack_reference(w), "first at flat 1 ", by_bits=True)


def test_planted_step_prologue_fault():
    for dtype in po.DTYPES:
        for rb in po.ROW_BYTES:
            tvals, table = po.step_table(rb, dtype)
            assert table.shape[1] * table.element_size() == rb
            for step in (0, 2, po.STEP_ROWS - 2):
                row, t, after = po.step_row_reference(tvals, table, step, pre_advance=True)
                assert after == step + 1 and float(t) == float(tvals[step + 1])
                stale, t_stale, _ = po.step_row_reference(tvals, table, step, pre_advance=False)     # the fault: row `step`
                _fails(stale, row, "first at flat 0 ", by_bits=True)
                assert float(t_stale) != float(t)
    # neighbouring rows differ in every 16-byte chunk's first element, also in bf16
    for rb in po.ROW_BYTES:
        _, table = po.step_table(rb, torch.bfloat16)
        assert po.addressed_strides_ok([table.shape[1]]) or rb == 16 * 1024 + 16
        assert not torch.equal(table[1], table[2])


def test_planted_masked_metrics_fault():
    for dtype in po.DTYPES:
        for n in po.METRIC_SIZES:
            a, b, m = po.metrics_case(n, dtype)
            ref = po.metrics_reference(a, b, m)
            assert ref[1].tolist() == [0.0] * 6                                   # the sample that is fully masked out
            assert float(ref[2, 2]) == 0.0 and float(ref[2, 4]) == 0.0 and float(a.float()[2].max()) < 0
            unmasked = ref.clone()
            unmasked[:, 2] = a.double().max(1).values                            # the fault: a maximum that ignores the mask
            if n > 1:
                _fails(unmasked, ref, "first at flat", names=("sample", "output"))
            assert float(ref.max()) < 2 ** 24                                     # every sum is an exact fp32 integer
    a, b, m = po.metrics_case(4099, torch.float32)
    msg = _fails(po.metrics_reference(a, b, torch.ones_like(m)), po.metrics_reference(a, b, m), "sample=0", names=("sample", "output"))
    assert "output=" in msg


# ------------------------------------------------------------------------------------------------ addressed values
def test_addressed_values():
    i = torch.arange(1 << 16)
    h = po.addressed(1 << 16, torch.bfloat16)
    assert torch.equal(h.float(), ((i % 251) - 125).float()) and float(h.float().abs().max()) == 125      # exact in bf16
    hf = h.float()
    for d in list(range(1, 251)) + [252, 256, 1000, 4095, 4096]:
        assert bool((hf[d:] != hf[:-d]).all()) == (d % 251 != 0), d
    # the displacements a wrong index moves an element by in the layout / pack / row cases: channel, pixel, tap and row strides
    for B, C, H, W in po.LAYOUT_SHAPES:
        assert po.addressed_strides_ok([1, C if C > 1 else 0, H * W if H * W > 1 else 0]), (B, C, H, W)
    for s in po.PACK_SHAPES:
        O, I, KK = s[0], s[1], (s[2] * s[3] if len(s) == 4 else 1)
        assert po.addressed_strides_ok([1, I if I > 1 else 0, KK if KK > 1 else 0]), s
    f = po.addressed(2 * po.GRID_REACH + 5, torch.float32)
    assert float(f[-1]) == 2 * po.GRID_REACH + 4 and bool((f[1:] - f[:-1] == 1).all())
    assert any(B * C * H * W == po.GRID_REACH for B, C, H, W in po.LAYOUT_SHAPES)
    assert any(B * C * H * W == 2 * po.GRID_REACH + 5 and C % 2 and (H * W) % 2 for B, C, H, W in po.LAYOUT_SHAPES)


def test_canary_buffers():
    buf, view = po.with_canaries((2, 3), torch.float32, "cpu")
    assert view.is_contiguous() and view.data_ptr() % 16 == buf.data_ptr() % 16
    view.copy_(torch.ones(2, 3))
    assert po.canaries_intact(buf, 6)
    buf[63] = 0
    assert not po.canaries_intact(buf, 6)


# ------------------------------------------------------------------------------------------------ tolerances
def test_embedding_tolerance_dominates_the_count():
    assert po.EMB_CONST_ERR + 2 <= po.EMB_E_REL and po.EMB_CONST_ERR <= 0.5
    a = torch.cat([torch.logspace(-12, math.log10(po.EMB_T_MAX), 20000, dtype=torch.float64), torch.tensor([600.0, po.EMB_T_MAX])])
    assert bool((po.emb_tolerance(a) >= po.emb_error_bound(a)).all())
    assert float(po.emb_tolerance(torch.tensor(1000.0, dtype=torch.float64))) <= 2e-4        # the bound of the first test
    assert float(po.emb_tolerance(torch.tensor(0.0, dtype=torch.float64))) <= 8.1e-5
    # the float64 reference is the formula: against torch's own fp32 embedding of the UNet oracle it differs by fp32 error only
    from oracle.unet import timestep_embedding
    t = torch.tensor([981.0, 501.0, 1.0])
    ref, a_abs = po.emb_reference(t, 192)
    assert po.worst_over_bound(timestep_embedding(t, 192), ref, po.emb_tolerance(a_abs))[0] <= 1.0
    lo, _ = po.emb_reference(t, 192, flip=False)
    assert torch.equal(lo[:, :96], ref[:, 96:]) and torch.equal(lo[:, 96:], ref[:, :96])
    r0, _ = po.emb_reference(torch.zeros(1), 6, freq_shift=1.0)
    assert r0.tolist() == [[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]]
    # a frequency off by one index is far outside the bound
    wrong, _ = po.emb_reference(t, 194)
    assert po.worst_over_bound(wrong[:, 1:97], ref[:, :96], po.emb_tolerance(a_abs[:, :96]))[0] > 100


def test_silu_tolerance():
    x = po.silu_points()
    assert x.numel() == 4096 + 6 and float(x.min()) == -100 and float(x.max()) == 100
    ref = po.silu_reference(x)
    tol = po.silu_tolerance(x, ref)
    assert po.SILU_CONST_ERR <= 0.5
    assert bool((tol <= po.U * ref.abs() * (po.SILU_C + 1.5 * x.double().abs()) + po.DENORM).all())   # the stated form, c = 6
    near = x.abs() <= 4
    assert float(tol[near].max()) <= 1e-6                                     # not looser than the first test of this kernel
    assert po.worst_over_bound(torch.nn.functional.silu(x[near]), ref[near], tol[near])[0] <= 1.0
    # x * sigmoid(x) with a sigmoid off by 2^-20 is caught
    assert po.worst_over_bound(ref * (1 + 2.0 ** -20), ref, tol)[0] > 1.0
    for v, want in ((math.inf, math.inf), (-math.inf, math.nan), (math.nan, math.nan)):
        got = float(po.silu_reference(torch.tensor([v]))[0])
        assert (math.isnan(got) and math.isnan(want)) or got == want


def test_ddim_reference_and_gather_row():
    g = torch.Generator().manual_seed(2)
    x, e = torch.randn(2, 3, 5, 5, generator=g), torch.randn(2, 3, 5, 5, generator=g)
    ref, scale = po.ddim_reference(x, e, po.DDIM_ROWS[1])
    sa_t, sb_t, sa_p, sb_p = (torch.tensor(v, dtype=torch.float32) for v in po.DDIM_ROWS[1])
    fp32 = sa_p * ((x - sb_t * e) / sa_t) + sb_p * e
    assert po.worst_over_bound(fp32, ref, po.ddim_tolerance(ref, scale))[0] <= 1.0
    for other in (0, 2):                                                      # a launch that read a sentinel row is far off
        bad, _ = po.ddim_reference(x, e, po.DDIM_ROWS[other])
        assert po.worst_over_bound(bad, ref, po.ddim_tolerance(ref, scale))[0] > 1e3
    eps = po.addressed(2 * 3 * 5 * 5, torch.float32).reshape(2, 5, 5, 3)       # NHWC
    out, _ = po.ddim_reference(torch.zeros(2, 3, 5, 5), po.nchw_reference(eps), po.DDIM_GATHER_ROW)
    assert torch.equal(out.float(), po.nchw_reference(eps))
    assert max(B * C * H * W for B, C, H, W in po.DDIM_SHAPES) == 658845 > po.GRID_REACH


def test_real_fir_tolerance_is_tight_enough_to_see_one_tap():
    from oracle import upfirdn as ou
    x, f = po.real_fir_case()
    f2 = torch.outer(f, f)
    pad = (6, 6, 6, 6)
    ref = ou.upfirdn2d(x.double(), f2, padding=list(pad))
    tol = po.real_fir_tolerance(x, f2, ref, pad, torch.float32)
    assert po.worst_over_bound(ou.upfirdn2d(x, f2, padding=list(pad)), ref, tol)[0] <= 1.0      # torch's fp32 conv fits
    f_bad = f2.clone()
    f_bad[0, 0] = 0                                                           # the smallest corner tap, ~1e-4 of the centre
    assert po.worst_over_bound(ou.upfirdn2d(x.double(), f_bad, padding=list(pad)), ref, tol)[0] > 1.0
