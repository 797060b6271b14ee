"""Flow-guided interpolation on MI355X: the forward bilinear splat (afldm_flow_splat) against the CPU oracle of
tests/flow_oracle.py within the DERIVED bound (k + 1) 2^-23 mag per target, the backward sampler (afldm_flow_warp) against
float64 F.grid_sample, the reference's recorded outputs (tests/golden/g17_flow.npz), and LDMInterpolationPipeline with
warp_method 0 / 1 / 2: the batched path against the per-frame reference loop."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_oracle as fo

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_flow.npz")
EPS = 2.0 ** -23


def smooth_flow(H, A, sign):
    """f0 = sign A sin(2 pi (i/H + 0.3 j/H) + 0.4), f1 = sign A cos(2 pi (j/H - 0.2 i/H) + 1.1): [2, H, H] fp32, channel 0 = rows.
    The negative sign drives sources across the top and left borders (negative coefficients, targets with cnt < 0)."""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
    return np.stack([sign * A * np.sin(2 * np.pi * (i / H + 0.3 * j / H) + 0.4),
                     sign * A * np.cos(2 * np.pi * (j / H - 0.2 * i / H) + 1.1)]).astype(np.float32)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device="cuda", dtype=dtype).contiguous()


def within(got, want, bound, what):
    """|got - want| <= bound elementwise; prints the largest used fraction of the bound before asserting."""
    got, want, bound = (np.asarray(a, dtype=np.float64) for a in (got, want, bound))
    err = np.abs(got - want)
    used = float(np.max(err / np.maximum(bound, 1e-300), initial=0.0, where=err > 0))
    print(f"[{what}] max |err| {err.max():.3e}, largest fraction of the bound used {used:.3f}")
    assert np.all(err <= bound), (what, float(err.max()), used)


# ------------------------------------------------------------------------------------------------- splat vs oracle
@pytest.mark.parametrize("B", [1, 15])
@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("H,A", [(32, 2.0), (64, 3.0), (256, 12.0)])
def test_splat_vs_oracle(H, A, sign, B):
    """fp32; pick mode at ds 1 and 8 and pool mode at ds 8, each with and without fill; B samples over ONE shared source and
    flow with per-sample scales.  res and the pooled sums within the derived bound, occ equal outside the oracle's ambiguous
    set, which may hold at most 0.1 % of the targets and is empty for the (64, 3) and (256, 12) flows."""
    from afldm_amd import ops
    C, ds = 4, 8
    rng = np.random.default_rng(H + B)
    x = rng.standard_normal((C, H, H)).astype(np.float32)
    flow = smooth_flow(H, A, sign)
    scales = np.array([0.625], dtype=np.float32) if B == 1 else torch.linspace(0, 1, 17)[1:-1].numpy()
    fill1 = rng.standard_normal((1, C, H, H)).astype(np.float32)          # one shared full-resolution draw (pick)
    fillB = rng.standard_normal((B, C, H, H)).astype(np.float32)          # a draw per sample (pool)
    orc = [fo.splat(x, flow, s) for s in scales]
    amb = np.stack([o["ambiguous"] for o in orc])
    occ_frac = float(np.mean([o["occ"].mean() for o in orc]))
    print(f"[splat {H} A {A} sign {sign:+.0f} B {B}] ambiguous {int(amb.sum())}, occluded {occ_frac:.3%}, cnt < 0 "
          f"{np.mean([(o['cnt'] < 0).mean() for o in orc]):.3%}")
    assert amb.mean() <= 1e-3
    if H in (64, 256):
        assert not amb.any()
        if B == 15:
            assert occ_frac >= 0.01          # the fill path is exercised
    xd, fd, sd = dev(x[None]), dev(flow[None]), dev(scales)
    for d in (1, ds):
        for fill in (None, fill1):
            res, occ = ops.flow_splat(xd, fd, sd, ds=d, mode=ops.FLOW_PICK, fill=None if fill is None else dev(fill),
                                      fill_pix_stride=d)
            assert res.shape == (B, C, H // d, H // d) and occ.shape == (B, 1, H // d, H // d)
            res, occ = res.cpu().numpy(), occ.cpu().numpy()
            for b, o in enumerate(orc):
                want, bound, wocc, wamb = fo.pick(o, d, None if fill is None else fill[0])
                keep = ~wamb
                assert np.array_equal((occ[b, 0] > 0.5)[keep], wocc[keep]) and set(np.unique(occ)) <= {0.0, 1.0}
                if b in (0, B // 2, B - 1):
                    within(res[b][:, keep], want[:, keep], bound[:, keep], f"pick ds {d} fill {fill is not None} b {b}")
                else:
                    assert np.all(np.abs(res[b][:, keep] - want[:, keep]) <= bound[:, keep]), (d, b)
    for fill in (None, fillB):
        res, occ = ops.flow_splat(xd, fd, sd, ds=ds, mode=ops.FLOW_POOL, fill=None if fill is None else dev(fill))
        assert res.shape == (B, C, H // ds, H // ds) and occ.shape == (B, 1, H, H)
        res, occ = res.cpu().numpy(), occ.cpu().numpy()
        for b, o in enumerate(orc):
            want, bound = fo.pool(o, ds, None if fill is None else fill[b])
            keep = ~o["ambiguous"].reshape(H // ds, ds, H // ds, ds).any(axis=(1, 3))
            assert np.array_equal((occ[b, 0] > 0.5)[~o["ambiguous"]], o["occ"][~o["ambiguous"]])
            within(res[b][:, keep], want[:, keep], bound[:, keep], f"pool ds {ds} fill {fill is not None} b {b}")


def test_splat_identity_integer_shift_and_bf16():
    """Zero flow: the identity, occ = 0.  Integer flow: a shifted copy, bit for bit (every non-zero coefficient is exactly 1),
    occ = 1 exactly where nothing lands.  bf16: the fp32 result of the bf16-rounded input, rounded once."""
    from afldm_amd import ops
    from afldm_amd.shift_utils import flow_utils as fu
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 64, 64, generator=g).cuda()
    res, occ = fu.forward_flow_warp(x, torch.zeros(2, 2, 64, 64, device="cuda"))
    assert torch.equal(res, x) and not occ.any()
    flow = torch.zeros(2, 2, 64, 64, device="cuda")
    flow[:, 0], flow[:, 1] = 3.0, -2.0
    res, occ = fu.forward_flow_warp(x, flow)
    want, wocc = torch.zeros_like(x), torch.ones(2, 1, 64, 64, device="cuda")
    want[:, :, 3:, :-2], wocc[:, :, 3:, :-2] = x[:, :, :-3, 2:], 0.0
    assert torch.equal(res, want) and torch.equal(occ, wocc)
    # per-sample scale on an integer flow: sample b is shifted by b rows
    one = torch.zeros(1, 2, 64, 64, device="cuda")
    one[:, 0] = 1.0
    res, _ = fu.forward_flow_warp_frames(x[:1], one, [0.0, 1.0, 2.0, 5.0])
    for b, s in enumerate((0, 1, 2, 5)):
        assert torch.equal(res[b, :, s:], x[0, :, :64 - s])
    xb = x.to(torch.bfloat16)
    f = torch.from_numpy(smooth_flow(64, 3.0, -1.0))[None].repeat(2, 1, 1, 1).cuda()
    rb, ob = fu.forward_flow_warp(xb, f)
    rf, of = fu.forward_flow_warp(xb.float(), f)
    assert rb.dtype == ob.dtype == torch.bfloat16 and torch.equal(ob.float(), of)
    o = [fo.splat(xb[b].float().cpu().numpy(), f[b].cpu().numpy()) for b in range(2)]
    want, bound = np.stack([a["res"] for a in o]), np.stack([a["bound"] for a in o])
    within(rb.float().cpu().numpy(), want, bound + 2.0 ** -8 * (np.abs(want) + bound), "bf16 splat")
    with pytest.raises(ValueError):
        ops.flow_splat(x, flow, torch.ones(2, device="cuda"), ds=5)
    with pytest.raises(ValueError):
        ops.flow_splat(x, flow[:, :, :32].contiguous(), torch.ones(2, device="cuda"))
    with pytest.raises(RuntimeError):
        fu.forward_flow_warp(x.cpu(), flow.cpu())
    from afldm_amd._lib import AfldmError
    with pytest.raises(AfldmError, match="65535"):          # one sample per grid row: refused with the limit named
        ops.flow_splat(x[:1, :1, :8, :8].contiguous(), flow[:1, :, :8, :8].contiguous(), torch.ones(65536, device="cuda"))


def test_splat_fixture_cases():
    """The reference's recorded outputs.  The reference sums in fp32 in source order, the kernel in fp32 in arrival order:
    two fp32 sums of the same k terms each err by at most (k - 1) 2^-24 mag to first order, so they differ by less than the
    bound (k + 1) 2^-23 mag itself; occ equal (the oracle's ambiguous set is empty for these cases)."""
    from afldm_amd.af_libs.ideal_lpf import UpsampleRFFT
    from afldm_amd.shift_utils import flow_utils as fu
    z = np.load(GOLDEN)
    for name in ("rand32", "neg64"):
        x, flow = z[f"splat_{name}_x"], z[f"splat_{name}_flow"]
        o = fo.splat(x[0], flow[0])
        assert not o["ambiguous"].any()
        res, occ = fu.forward_flow_warp(dev(x), dev(flow))
        assert np.array_equal(occ.cpu().numpy(), z[f"splat_{name}_occ"])
        within(res.cpu().numpy()[0], o["res"], o["bound"], f"fixture {name} vs oracle")
        within(res.cpu().numpy()[0], z[f"splat_{name}_res"][0], o["bound"], f"fixture {name} vs reference")
    # forward_upsample_flow_warp: our ideal up-sampling feeds the oracle; against the reference's record the difference of the
    # two up-samplers (FFT there, a matrix product here: bounded by 16 roundings of the 8-point sums, 2^-19 max|x|) enters
    # every target through sum |coef|
    x, flow = z["upwarp_x"], z["upwarp_flow"]
    hi = UpsampleRFFT(8)(dev(x))
    o = fo.splat(hi[0].cpu().numpy(), flow[0])
    assert not o["ambiguous"].any()
    res, occ = fu.forward_upsample_flow_warp(dev(x), dev(flow), scale=8)
    want, bound, wocc, _ = fo.pick(o, 8)
    assert res.shape == (1, 2, 8, 8) and np.array_equal(occ.cpu().numpy()[0, 0] > 0.5, wocc)
    assert np.array_equal(occ.cpu().numpy(), z["upwarp_occ"])
    within(res.cpu().numpy()[0], want, bound, "upsample + warp vs oracle")
    slack = 2.0 ** -19 * float(np.abs(hi.cpu().numpy()).max()) * o["cmag"][::8, ::8]
    within(res.cpu().numpy()[0], z["upwarp_res"][0], bound + slack[None], "upsample + warp vs reference")


def test_noise_helpers_fixture_cases():
    """upsample_noise, collect_noise_pixel and continuous_noise_fwd_warp with the reference's own draws fed in."""
    from afldm_amd.shift_utils import flow_utils as fu
    z = np.load(GOLDEN)
    hi = fu.upsample_noise(dev(z["upnoise_x"]), 8, noise_draw=dev(z["upnoise_z"]))
    # x / 8 + z - mean(z): three roundings of values below max|z| + max|x|, and the 64-term mean
    assert np.abs(hi.cpu().numpy() - z["upnoise_y"]).max() <= 66 * EPS * (np.abs(z["upnoise_z"]).max() + np.abs(z["upnoise_x"]).max())
    hi = dev(z["upnoise_y"])
    y = fu.collect_noise_pixel(hi, dev(z["collect_occ"]), 8, noise_draw=dev(z["collect_z"]))
    terms = np.abs(np.where(z["collect_occ"] > 0.5, z["collect_z"], z["upnoise_y"])).reshape(1, 2, 4, 8, 4, 8).sum(axis=(3, 5))
    within(y.cpu().numpy(), z["collect_y"], 65 * EPS * terms / 8, "collect_noise_pixel vs reference")
    flow, alpha = z["cnfw_flow"], float(z["cnfw_alpha"])
    o = fo.splat(z["upnoise_y"][0], flow[0], alpha)
    assert not o["ambiguous"].any() and o["occ"].mean() > 0.01
    want, bound = fo.pool(o, 8, z["cnfw_z"][0])
    for a in (alpha, torch.tensor(alpha)):
        y = fu.continuous_noise_fwd_warp(hi, dev(flow), a, 8, noise=dev(z["cnfw_z"]))
        within(y.cpu().numpy()[0], want, bound, "continuous_noise_fwd_warp vs oracle")
        within(y.cpu().numpy()[0], z["cnfw_y"][0], bound, "continuous_noise_fwd_warp vs reference")
    # generator: a CPU generator draws what torch.randn draws on the CPU
    y = fu.continuous_noise_fwd_warp(hi, dev(flow), alpha, 8, generator=torch.Generator().manual_seed(9))
    draw = torch.randn(hi.shape, generator=torch.Generator().manual_seed(9))
    want, bound = fo.pool(o, 8, draw[0].numpy())
    within(y.cpu().numpy()[0], want, bound, "continuous_noise_fwd_warp, seeded generator")


@pytest.mark.parametrize("H,A", [(64, 3.0), (256, 12.0)])
def test_splat_batched_vs_single_and_graph_replay(H, A):
    """One launch over 15 samples against 15 single-sample launches: the sums are atomic, so two runs agree to summation
    order (not torch.equal): two fp32 sums of the same k terms differ by at most (k - 1) 2^-23 mag to first order, which is
    inside the bound (k + 1) 2^-23 mag, so they are held to the same bound of each other; occ equal.  A captured call replays
    new `scale` values."""
    from afldm_amd import ops
    C, ds, B = 4, 8, 15
    rng = np.random.default_rng(7)
    x, flow = rng.standard_normal((C, H, H)).astype(np.float32), smooth_flow(H, A, -1.0)
    scales = torch.linspace(0, 1, 17)[1:-1].numpy()
    fill = rng.standard_normal((1, C, H, H)).astype(np.float32)
    orc = [fo.splat(x, flow, s) for s in scales]
    assert not any(o["ambiguous"].any() for o in orc)
    xd, fd, bg = dev(x[None]), dev(flow[None]), dev(fill)
    res, occ = ops.flow_splat(xd, fd, dev(scales), ds=ds, fill=bg, fill_pix_stride=ds)
    for b, o in enumerate(orc):
        r1, o1 = ops.flow_splat(xd, fd, dev(scales[b:b + 1]), ds=ds, fill=bg, fill_pix_stride=ds)
        assert torch.equal(o1[0], occ[b])
        bound = fo.pick(o, ds, fill[0])[1]
        assert np.all(np.abs((r1[0] - res[b]).cpu().numpy()) <= bound), b
    # capture, then replay with other scales
    sc = dev(scales)
    out, oc = torch.empty_like(res), torch.empty_like(occ)
    ws = torch.empty(ops.flow_splat_workspace(B, C, H, H, ds, ops.FLOW_PICK), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.flow_splat(xd, fd, sc, ds=ds, fill=bg, fill_pix_stride=ds, out=out, occ=oc, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.flow_splat(xd, fd, sc, ds=ds, fill=bg, fill_pix_stride=ds, out=out, occ=oc, workspace=ws)
    for new in (scales[::-1].copy(), scales * 0.5):
        sc.copy_(torch.from_numpy(new))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        for b in (0, 7, 14):
            o = fo.splat(x, flow, new[b])
            want, bound, wocc, wamb = fo.pick(o, ds, fill[0])
            assert np.array_equal((oc[b, 0] > 0.5).cpu().numpy()[~wamb], wocc[~wamb])
            assert np.all((np.abs(out[b].cpu().numpy() - want) <= bound)[:, ~wamb]), b


# ------------------------------------------------------------------------------------------------- backward sampler
def _grid64(flow):
    """The reference's grid (flow_utils.py:53-86) with its fp32 operations on the CPU: coords_grid + flip(flow), normalised by
    2 c / (n - 1) - 1; returns (grid [B, H, W, 2] fp32, mask)."""
    B, _, H, W = flow.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    coords = torch.stack([xs, ys]).float()[None] + torch.flip(flow, (1,))
    xg, yg = 2 * coords[:, 0] / (W - 1) - 1, 2 * coords[:, 1] / (H - 1) - 1
    return torch.stack([xg, yg], dim=-1), (xg >= -1) & (yg >= -1) & (xg <= 1) & (yg <= 1)


@pytest.mark.parametrize("H", [32, 64, 256])
def test_flow_warp_vs_grid_sample(H):
    """Bilinear against float64 F.grid_sample on the same flipped, normalised grid.  The fp32 normalise / un-normalise round
    trip moves a coordinate by at most delta = 4 (W - 1) 2^-24 pixels and a bilinear sample changes by at most 2 max|x| per
    pixel of coordinate and axis: |y - y64| <= (4 delta + 8 2^-24) max|x| in fp32, one bf16 rounding more in bf16.  The mask
    equal; integer flows bit for bit; nearest exact on integer + 0.25 fields."""
    from afldm_amd.shift_utils import flow_utils as fu
    g = torch.Generator().manual_seed(H)
    B, C = 2, 3
    x = torch.randn(B, C, H, H, generator=g)
    flow = torch.randn(B, 2, H, H, generator=g) * (H / 16)
    flow[0, :, :4] = torch.randint(-6, 7, (2, 4, H), generator=g).float()          # integer landings incl. the exact borders
    grid, wmask = _grid64(flow)
    delta = 4 * (H - 1) * 2.0 ** -24
    for dtype in (torch.float32, torch.bfloat16):
        xq = x.to(dtype)
        want = F.grid_sample(xq.double(), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=True).numpy()
        y, m = fu.flow_warp(xq.cuda(), flow.cuda(), mask=True)
        assert y.dtype == dtype and m.dtype == torch.bool and torch.equal(m.cpu(), wmask)
        bound = (4 * delta + 8 * 2.0 ** -24) * float(xq.abs().max())
        tol = bound if dtype == torch.float32 else bound + 2.0 ** -8 * (np.abs(want) + bound)
        within(y.float().cpu().numpy(), want, np.broadcast_to(tol, want.shape), f"flow_warp {H} {dtype}")
        assert torch.equal(fu.flow_warp(xq.cuda(), flow.cuda()), y)
        # bilinear_sample: the coordinates themselves (channel 0 = x), both layouts
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(H), indexing="ij")
        coords = (torch.stack([xs, ys]).float()[None] + torch.flip(flow, (1,))).cuda()
        y2, m2 = fu.bilinear_sample(xq.cuda(), coords, return_mask=True)
        assert torch.equal(y2, y) and torch.equal(m2, m)
        assert torch.equal(fu.bilinear_sample(xq.cuda(), coords.permute(0, 2, 3, 1)), y)
        # integer flow: a shifted copy with zero padding, bit for bit
        iflow = torch.zeros(B, 2, H, H)
        iflow[:, 0], iflow[:, 1] = 2.0, -3.0
        yi, mi = fu.flow_warp(xq.cuda(), iflow.cuda(), mask=True)
        wi, wm = torch.zeros_like(xq), torch.zeros(B, H, H, dtype=torch.bool)
        wi[:, :, :-2, 3:], wm[:, :-2, 3:] = xq[:, :, 2:, :-3], True
        assert torch.equal(yi.cpu(), wi) and torch.equal(mi.cpu(), wm)
        # nearest on integer + 0.25: exact
        qflow = torch.randint(-5, 6, (B, 2, H, H), generator=g).float() + 0.25
        wn = F.grid_sample(xq.double(), _grid64(qflow)[0].double(), mode="nearest", padding_mode="zeros", align_corners=True)
        assert torch.equal(fu.flow_warp(xq.cuda(), qflow.cuda(), mode="nearest").cpu().double(), wn)
    with pytest.raises(NotImplementedError):
        fu.flow_warp(x.cuda(), flow.cuda(), padding_mode="border")
    with pytest.raises(RuntimeError):
        fu.flow_warp(x, flow)


def test_flow_warp_and_consistency_check_fixture_cases():
    from afldm_amd.shift_utils import flow_utils as fu
    z = np.load(GOLDEN)
    x, flow = z["warp_x"], z["warp_flow"]
    y, m = fu.flow_warp(dev(x), dev(flow), mask=True)
    assert np.array_equal(m.cpu().numpy(), z["warp_mask"])
    # the reference's fp32 grid_sample is within the sampler bound of the exact sample; the kernel samples at the pixel
    # coordinate itself (no round trip), so it adds only the 8 2^-24 max|x| of the interpolation arithmetic
    bound = (4 * 4 * 31 * 2.0 ** -24 + 2 * 8 * 2.0 ** -24) * float(np.abs(x).max())
    within(y.cpu().numpy(), z["warp_y"], np.broadcast_to(bound, y.shape), "flow_warp vs reference")
    assert np.array_equal(fu.flow_warp(dev(x), dev(z["warp_qflow"]), mode="nearest").cpu().numpy(), z["warp_ynear"])
    # get_patch_moving_flow
    tmpl = torch.zeros(1, 3, 64, 64, device="cuda")
    box, disp = tuple(int(v) for v in z["patch_box"]), tuple(int(v) for v in z["patch_disp"])
    bwd, bwd_occ = fu.get_patch_moving_flow(tmpl, box, disp)
    half, half_occ = fu.get_patch_moving_flow(tmpl, box, disp, alpha=0.5)
    for got, name in ((bwd, "patch_bwd"), (bwd_occ, "patch_bwd_occ"), (half, "patch_half"), (half_occ, "patch_half_occ")):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), z[name]), name
    # forward_backward_consistency_check on the consistent pair.  First, on a float64 restatement: no pixel's diff lies within
    # the sampler bound (of a flow field: max|x| = the displacement) of its threshold, so the comparison leaves nothing out
    fwd = torch.from_numpy(z["patch_fwd"])
    bw = torch.from_numpy(z["patch_bwd"])
    sb = (4 * 4 * 63 * 2.0 ** -24 + 8 * 2.0 ** -24) * float(max(fwd.abs().max(), bw.abs().max())) * 2 ** 0.5
    for a, b in ((fwd, bw), (bw, fwd)):
        warped = F.grid_sample(b.double(), _grid64(a)[0].double(), mode="bilinear", padding_mode="zeros", align_corners=True)
        diff = torch.norm(a.double() + warped, dim=1)
        thr = 0.01 * (torch.norm(a.double(), dim=1) + torch.norm(b.double(), dim=1)) + 0.5
        assert float((diff - thr).abs().min()) > sb + 1e-5
    f_occ, b_occ = fu.forward_backward_consistency_check(fwd.cuda(), bw.cuda())
    assert f_occ.shape == (1, 1, 64, 64) and np.array_equal(f_occ.cpu().numpy(), z["fb_fwd_occ"])
    assert np.array_equal(b_occ.cpu().numpy(), z["fb_bwd_occ"]) and 0 < float(z["fb_fwd_occ"].mean()) < 1
    # flow_warp_with_occ_bg: both filters, the background fed in
    img = dev(x[:1])
    mask = (torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(1)) < 0.8).float().cuda()
    bgn = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    got = fu.flow_warp_with_occ_bg(img, dev(flow[:1]), mask, True, noise=bgn)
    assert torch.equal(got, fu.flow_warp(img, dev(flow[:1])) * mask + bgn * (1 - mask))
    g1 = fu.flow_warp_with_occ_bg(img, dev(flow[:1]), mask, True, generator=torch.Generator().manual_seed(2))
    assert torch.equal(g1, got)
    # the colour background is drawn where the generator lives: a CPU and a device generator both work
    for gdev in ("cpu", "cuda"):
        c1 = fu.flow_warp_with_occ_bg(img, dev(flow[:1]), mask, False, generator=torch.Generator(device=gdev).manual_seed(4))
        bgc = torch.rand((1, 3, 1, 1), generator=torch.Generator(device=gdev).manual_seed(4), device=gdev).cuda() * 2 - 1
        assert torch.equal(c1, fu.flow_warp(img, dev(flow[:1])) * mask + bgc * (1 - mask))
    const = torch.zeros(1, 2, 32, 32, device="cuda")
    const[:, 0], const[:, 1] = 1.5, -2.25
    from afldm_amd.af_libs.equivariance import apply_fractional_translation
    lz = fu.flow_warp_with_occ_bg(img, const, mask, False, "lanczos", noise=torch.full((1, 3, 1, 1), 0.5))
    assert torch.equal(lz, apply_fractional_translation(img, 2.25 / 32, -1.5 / 32)[0] * mask + 0.5 * (1 - mask))


# ------------------------------------------------------------------------------------------------- pipeline
def _patch_flows(S):
    """(fwd_flow, bwd_flow) [1, 2, S, S] in the pipeline's input convention (channel 0 = x) of a patch moved by (di, dj), from
    get_patch_moving_flow: the backward flow lives on the moved patch, the forward flow on the original one."""
    from afldm_amd.shift_utils import flow_utils as fu
    tmpl = torch.zeros(1, 3, S, S, device="cuda")
    u, d, l, r = S // 4, S // 4 + S // 3, S // 2, S // 2 + S // 3
    di, dj = S // 5, -(S // 4)
    bwd = fu.get_patch_moving_flow(tmpl, (u, d, l, r), (di, dj))[0]
    fwd = fu.get_patch_moving_flow(tmpl, (u + di, d + di, l + dj, r + dj), (-di, -dj))[0]
    assert float(fwd[0, 0, u, l]) == di and float(bwd[0, 1, u + di, l + dj]) == -dj
    return torch.flip(fwd, (1,)), torch.flip(bwd, (1,))


def _smooth_flows(S):
    f = torch.from_numpy(smooth_flow(S, S * 3.0 / 64, -1.0))[None].cuda()
    return torch.flip(f, (1,)), torch.flip(-f, (1,))


def _slerp_tolerance(a, da, b, db, t):
    """Elementwise bound on the change of slerp(a, b, t) = w0 a + w1 b (float64, rounded to fp32) when a and b move by at most
    da and db elementwise: |w0| da + |w1| db, plus the change of the weights: the cosine of the angle between the normalised
    tensors moves by at most dcos = 2 (|da| / |a| + |db| / |b|) (norms), and the weights are evaluated at cos -+ dcos; plus
    the two fp32 roundings of the results."""
    from afldm_amd.pipelines.image_interpolation_pipeline import _arc_weights
    a, da, b, db = (torch.as_tensor(v).double() for v in (a, da, b, db))
    cos = (torch.sum(a * b) / (torch.linalg.norm(a) * torch.linalg.norm(b))).clamp(-1 + 1e-7, 1 - 1e-7)
    dcos = 2 * (torch.linalg.norm(da) / torch.linalg.norm(a) + torch.linalg.norm(db) / torch.linalg.norm(b))
    w0, w1 = _arc_weights(cos, t)
    dw0 = max(abs(_arc_weights((cos + s * dcos).clamp(-1 + 1e-7, 1 - 1e-7), t)[0] - w0) for s in (-1, 1))
    dw1 = max(abs(_arc_weights((cos + s * dcos).clamp(-1 + 1e-7, 1 - 1e-7), t)[1] - w1) for s in (-1, 1))
    out = (w0 * a + w1 * b).abs()
    return w0.abs() * da + w1.abs() * db + dw0 * a.abs() + dw1 * b.abs() + 2 * EPS * (out + da + db)


def _frame_bounds(pipe, method, z0, z1, flows, n, seed):
    """Per intermediate frame: (warped_1, bound_1, warped_2, bound_2) from the CPU oracle on the inputs the pipeline forms
    (the same up-sampling calls and the same generator draws in the same order), after asserting that the oracle's ambiguous
    set is empty at every frame's scale.  Also returns the occluded fraction of the kept targets."""
    from afldm_amd.af_libs.ideal_lpf import UpsampleRFFT
    from afldm_amd.shift_utils import flow_utils as fu
    from afldm_amd.utils import randn_tensor
    ds = pipe.vae_scale_factor
    g = torch.Generator().manual_seed(seed)
    f_flow, b_flow = (torch.flip(f.float(), (1,)) for f in flows)
    if method == 1:
        hi = [fu.upsample_noise(z, ds, generator=g) for z in (z0, z1)]
    else:
        hi = [UpsampleRFFT(ds)(z) for z in (z0, z1)]
    bg = randn_tensor(tuple(hi[0].shape), generator=g, device="cuda", dtype=hi[0].dtype)
    alphas = torch.linspace(0, 1, n)
    rows, occluded = [], []
    for i in range(1, n - 1):
        row = []
        for e, (flow, s) in enumerate(((f_flow, alphas[i]), (b_flow, 1 - alphas[i]))):
            if method == 2:
                src = (z0, z1)[e][0].cpu().numpy()
                fl = F.interpolate(flow / ds, scale_factor=1 / ds, mode="nearest")[0].cpu().numpy()
            else:
                src, fl = hi[e][0].cpu().numpy(), flow[0].cpu().numpy()
            o = fo.splat(src, fl, float(s))
            assert not o["ambiguous"].any(), (method, i, e)
            if method == 0:
                want, bound, occ, _ = fo.pick(o, ds, bg[0].cpu().numpy())
                occluded.append(occ.mean())
            elif method == 1:
                fill = randn_tensor(tuple(hi[0].shape), generator=g, device="cuda", dtype=hi[0].dtype)
                want, bound = fo.pool(o, ds, fill[0].cpu().numpy())
                occluded.append(o["occ"].mean())
            else:
                want, bound = o["res"], o["bound"]
                occluded.append(o["occ"].mean())
            row += [want, bound]
        rows.append(row)
    return rows, float(np.mean(occluded)), g.get_state()


@pytest.mark.parametrize("flow_kind", ["patch", "smooth"])
@pytest.mark.parametrize("method", [0, 1, 2])
def test_pipeline_warp_methods_graph_vs_eager(method, flow_kind):
    """Tiny UNet + tiny AF-VAE, 5 frames, 6 steps, fp32, a seeded generator.  The batched path's initial frames against the
    per-frame loop's within the splat bound propagated through the slerp; both consume the generator identically; the final latents of the two paths within rel-RMS 1e-4; frames 0 / n-1 start as the inverted latents and
    end as the warp_method=3 call's (endpoints are never warped)."""
    from test_gpu_interp import _images, _tiny_pipeline, rel_rms
    n, steps, seed = 5, 6, 1234
    pipe, _ = _tiny_pipeline(torch.float32)
    images = _images(128)
    S = pipe.unet.config.sample_size * pipe.vae_scale_factor
    flows = _patch_flows(S) if flow_kind == "patch" else _smooth_flows(S)
    lat = pipe.image2latent(torch.cat(images)).float()
    pipe.scheduler.set_timesteps(steps)
    inv = pipe.ddim_inversion(lat, bar=False)
    z0, z1 = inv[0:1], inv[1:2]
    rows, occluded, state = _frame_bounds(pipe, method, z0, z1, flows, n, seed)
    print(f"[pipeline method {method} {flow_kind}] occluded targets {occluded:.3%}")
    if flow_kind == "patch":
        assert occluded >= 0.01
    gb, ge = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
    fb = pipe.initial_frames(z0, z1, n, method, flows, generator=gb, batched=True)
    fe = pipe.initial_frames(z0, z1, n, method, flows, generator=ge, batched=False)
    assert torch.equal(gb.get_state(), ge.get_state()) and torch.equal(gb.get_state(), state)
    fracs = [float(a) for a in torch.linspace(0, 1, n)]
    for frames in (fb, fe):
        assert torch.equal(frames[0], z0[0]) and torch.equal(frames[-1], z1[0])
    for i in range(1, n - 1):
        w1, b1, w2, b2 = rows[i - 1]
        tol = _slerp_tolerance(w1, b1, w2, b2, fracs[i]).numpy()
        within(fb[i].cpu().numpy(), fe[i].cpu().numpy(), tol, f"initial frame {i}, batched vs per frame")
        # and each against the oracle's own slerp
        from afldm_amd.pipelines.image_interpolation_pipeline import slerp
        want = slerp(torch.from_numpy(w1), torch.from_numpy(w2), fracs[i]).numpy()
        half = _slerp_tolerance(w1, b1, w2, b2, fracs[i]).numpy()
        within(fb[i].cpu().numpy(), want, half, f"initial frame {i}, batched vs oracle")
        within(fe[i].cpu().numpy(), want, half, f"initial frame {i}, per frame vs oracle")
    kw = dict(num_frames=n, num_inference_steps=steps, output_type="latent")
    g = pipe(*images, warp_method=method, flows=flows, generator=torch.Generator().manual_seed(seed), **kw)
    e = pipe(*images, warp_method=method, flows=flows, generator=torch.Generator().manual_seed(seed), use_graph=False, **kw)
    r = rel_rms(g, e)
    print(f"[pipeline method {method} {flow_kind}] final latents, graph vs eager: {r:.2e}")
    assert r <= 1e-4
    base = pipe(*images, **kw)
    assert rel_rms(g[0:1], base[0:1]) <= 1e-4 and rel_rms(g[-1:], base[-1:]) <= 1e-4
    assert rel_rms(g[1:-1], base[1:-1]) > 1e-3          # the warp moved the intermediate frames


def test_pipeline_zero_flow_method2_is_warp_method3_and_rejections():
    """Method 2 with a zero flow pair is the identity warp: warp_method=3's frames to slerp rounding."""
    from test_gpu_interp import _images, _tiny_pipeline
    pipe, _ = _tiny_pipeline(torch.float32)
    images = _images(128)
    zero = (torch.zeros(1, 2, 128, 128, device="cuda"), torch.zeros(1, 2, 128, 128, device="cuda"))
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(5)).cuda()
    from afldm_amd.pipelines.image_interpolation_pipeline import interp_alphas
    base = pipe._frames(z[0:1], z[1:2], 5, interp_alphas(5)[0], True)
    for batched in (True, False):
        got = pipe.initial_frames(z[0:1], z[1:2], 5, 2, zero, batched=batched)
        assert torch.all((got - base).abs() <= 2 * EPS * base.abs())
    kw = dict(num_frames=5, num_inference_steps=3, output_type="latent")
    from test_gpu_interp import rel_rms
    a, b = pipe(*images, warp_method=2, flows=zero, **kw), pipe(*images, **kw)
    assert rel_rms(a, b) <= 1e-4          # the graph-path tolerance of test_gpu_interp.py
    with pytest.raises(NotImplementedError, match="GMFlow"):
        pipe(*images, warp_method=0, **kw)
    with pytest.raises(ValueError, match="fwd_flow"):
        pipe(*images, warp_method=0, flows=(torch.zeros(1, 2, 64, 64), zero[1]), **kw)
    with pytest.raises(ValueError, match="pair"):
        pipe(*images, warp_method=1, flows=(zero[0],), **kw)
