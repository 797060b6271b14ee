"""The built-in optical-flow estimator on MI355X (csrc/flowest.hip, shift_utils/flow_estimation.py) against its oracle
(tests/flowest_oracle.py): the same arithmetic in torch on the CPU.

Tolerance: none is fixed in advance.  For every case delta = max |oracle_fp32 - oracle_fp64| on the same (fp32-representable)
input is the rounding scale of the computation itself; the HIP result must be within 8 delta of the fp64 oracle (the factor
covers a different order of the window sums and of the solve), and delta must stay below 1e-3 (px for a flow), so that a
degenerate delta cannot hide a failure.  Each case prints its ratio |hip - fp64| / delta."""
import pytest
import torch

import flowest_oracle as fo

pytestmark = pytest.mark.gpu

FACTOR, DELTA_MAX = 8.0, 1e-3


def rep(x):
    """fp64 tensor rounded to fp32-representable values (the fp64 and fp32 oracles and the GPU then see one input)."""
    return x.float().double()


def held(name, hip, ref64, ref32):
    delta = float((ref32.double() - ref64).abs().max())
    err = float((hip.double().cpu() - ref64).abs().max())
    print(f"[flowest {name}] delta {delta:.3e}  |hip - fp64| {err:.3e}  ratio {err / delta if delta else 0.0:.2f}")
    assert delta < DELTA_MAX, (name, delta)
    assert err <= FACTOR * delta, (name, err, delta)
    return delta


def planes(seed, n, H, W):
    return rep(fo.texture(seed, H, n, W))[0]                    # [n, H, W]


# ------------------------------------------------------------------------------------------------- single kernels
@pytest.mark.parametrize("H,W", [(16, 16), (40, 24)])
def test_pyr_down_vs_oracle(H, W):
    from afldm_amd import ops
    x = planes(3, 3, H, W)[None]
    y = ops.flowest_pyr_down(x.float().cuda())
    assert y.shape == (1, 3, H // 2, W // 2) and y.dtype == torch.float32
    held(f"pyr_down {H}x{W}", y, fo.pyr_down(x), fo.pyr_down(x.float()))
    yb = ops.flowest_pyr_down(x.bfloat16().cuda())              # a bf16 level reads the same planes rounded to bf16
    xb = x.bfloat16()
    held(f"pyr_down {H}x{W} bf16 in", yb, fo.pyr_down(xb.double()), fo.pyr_down(xb.float()))


def test_pyr_down_factor_1_converts():
    from afldm_amd import ops
    x = planes(4, 3, 40, 24)[None]
    for src in (x.bfloat16(), x.float()):
        y = ops.flowest_pyr_down(src.cuda(), factor=1)
        assert y.dtype == torch.float32 and y.shape == src.shape
        held(f"pyr_down factor 1 from {src.dtype}", y, src.double(), src.float())          # delta = 0: exact
    with pytest.raises(ValueError):
        ops.flowest_pyr_down(torch.zeros(1, 1, 15, 16, device="cuda"))
    with pytest.raises(ValueError):
        ops.flowest_pyr_down(torch.zeros(1, 1, 16, 16, device="cuda"), factor=3)


@pytest.mark.parametrize("H,W", [(8, 8), (20, 12), (64, 64)])
def test_smooth_and_up2_vs_oracle(H, W):
    from afldm_amd import ops
    u = rep(fo.smooth_field(5, 2, H, W, 3.0))
    ud = u.float().cuda()
    held(f"smooth {H}x{W}", ops.flowest_smooth(ud), fo.smooth(u), fo.smooth(u.float()))
    up = ops.flowest_up2(ud)
    assert up.shape == (2, 2, 2 * H, 2 * W)
    held(f"up2 {H}x{W}", up, fo.up2(u), fo.up2(u.float()))
    const = torch.full((1, 2, H, W), 1.25, device="cuda")       # a constant flow doubles under up2 and survives smoothing
    assert torch.equal(ops.flowest_up2(const), torch.full((1, 2, 2 * H, 2 * W), 2.5, device="cuda"))
    assert torch.equal(ops.flowest_smooth(const), const)


def lk_case(B, C, H, W):
    """(I1, I2, u) in fp64 at fp32-representable values: a texture, its translation by a per-sample sub-pixel shift, and an
    incoming flow of up to +-3 px that pushes samples across all four borders."""
    I1 = torch.stack([planes(10 + b, C, H, W) for b in range(B)])
    I2 = rep(torch.stack([fo.translate(I1[b], 1.3 - 2.0 * b, -0.8 + 1.1 * b) for b in range(B)]))
    u = rep(fo.smooth_field(20, B, H, W, 3.0))
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    assert (yy + u[:, 0]).min() < 0 and (yy + u[:, 0]).max() > H - 1 and (xx + u[:, 1]).min() < 0 and (xx + u[:, 1]).max() > W - 1
    return I1, I2, u


_LK_REF = {}


def lk_ref(B, C, H, W, r):
    """The oracle's step in fp64 and fp32, computed once per case and shared (never modified)."""
    key = (B, C, H, W, r)
    if key not in _LK_REF:
        I1, I2, u = lk_case(B, C, H, W)
        _LK_REF[key] = (I1, I2, u, fo.lk_step(I1, I2, u, r, 1e-3), fo.lk_step(I1.float(), I2.float(), u.float(), r, 1e-3))
    return _LK_REF[key]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("H,W", [(16, 16), (40, 24), (64, 64)])
def test_lk_step_vs_oracle(H, W, r, C, B):
    """One launch: 16^2 is one tile, 40 x 24 has overhanging tiles on a non-square plane, 64^2 several tiles."""
    from afldm_amd import ops
    I1, I2, u, ref64, ref32 = lk_ref(B, C, H, W, r)
    got = ops.flowest_lk_step(I1.float().cuda(), I2.float().cuda(), u.float().cuda(), r, 1e-3)
    held(f"lk_step {H}x{W} r{r} C{C} B{B}", got, ref64, ref32)
    assert float((got.cpu().double() - u).norm(dim=1).max()) <= 1.0 + 1e-5          # the step clamp


@pytest.mark.parametrize("H,W", [(16, 16), (40, 24), (64, 64), (72, 40)])
def test_lk_step_tiles_agree(H, W):
    """The 32 x 32 tile (one overhanging tile at 16^2 and 40 x 24, several at 64^2 and 72 x 40) against the oracle, and bit for
    bit against the 16 x 16 tile: the tile only partitions the work."""
    from afldm_amd import ops
    I1, I2, u, ref64, ref32 = lk_ref(2, 3, H, W, 3)
    args = (I1.float().cuda(), I2.float().cuda(), u.float().cuda(), 3, 1e-3)
    t32 = ops.flowest_lk_step(*args, tile=32)
    held(f"lk_step {H}x{W} tile 32", t32, ref64, ref32)
    assert torch.equal(t32, ops.flowest_lk_step(*args, tile=16)) and torch.equal(t32, ops.flowest_lk_step(*args))


def test_lk_step_chosen_tile_at_the_threshold_and_rejections():
    """512^2 x 2 is the first size at which the call picks the 32 x 32 tile itself (512 workgroups): equal to both forced
    tiles; 480 x 512 x 2 (480 workgroups) stays on 16 x 16."""
    from afldm_amd import ops
    for H in (512, 480):
        g = torch.Generator().manual_seed(H)
        I1 = (torch.rand(2, 1, H, 512, generator=g) * 2 - 1).cuda()
        I2 = (torch.rand(2, 1, H, 512, generator=g) * 2 - 1).cuda()
        u = (torch.rand(2, 2, H, 512, generator=g) * 6 - 3).cuda()
        auto = ops.flowest_lk_step(I1, I2, u)
        assert torch.equal(auto, ops.flowest_lk_step(I1, I2, u, tile=32)) and torch.equal(auto, ops.flowest_lk_step(I1, I2, u, tile=16))
        assert torch.isfinite(auto).all()
    z = torch.zeros(1, 2, 16, 16, device="cuda")
    from afldm_amd._lib import AfldmError
    for bad in (dict(radius=0), dict(radius=5), dict(lam=0.0), dict(tile=8), dict(out=z)):
        with pytest.raises(AfldmError):
            ops.flowest_lk_step(z, z.clone(), z, **bad)
    with pytest.raises(AfldmError):
        ops.flowest_lk_step(torch.zeros(1, 5, 16, 16, device="cuda"), torch.zeros(1, 5, 16, 16, device="cuda"), z)
    with pytest.raises(ValueError):
        ops.flowest_lk_step(z, z.clone(), torch.zeros(1, 2, 8, 8, device="cuda"))


# ------------------------------------------------------------------------------------------------- the whole estimator
def shifted_pair(seed, H, W, dy, dx):
    I1 = rep(fo.texture(seed, H, 3, W))
    return I1, rep(fo.translate(I1, dy, dx))


_EST_REF = {}


def est_ref(name, I1, I2, **kw):
    if name not in _EST_REF:
        _EST_REF[name] = (fo.bidirectional(I1, I2, **kw), fo.bidirectional(I1.float(), I2.float(), **kw))
    return _EST_REF[name]


@pytest.mark.parametrize("H,W,levels,shift", [(32, 32, 3, (1.5, -1.0)), (64, 64, 4, (3.5, -2.25)), (64, 32, 3, (2.0, 1.25))])
def test_estimator_vs_oracle(H, W, levels, shift):
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow
    I1, I2 = shifted_pair(0, H, W, *shift)
    (f64, b64), (f32, b32) = est_ref((H, W, levels), I1, I2, levels=levels)
    fwd, bwd = PyramidLKFlow(levels=levels)(I1.float().cuda(), I2.float().cuda())
    assert fwd.shape == bwd.shape == (1, 2, H, W) and fwd.dtype == torch.float32
    held(f"estimate {H}x{W} L{levels}", torch.cat([fwd, bwd]), torch.cat([f64, b64]), torch.cat([f32, b32]))


def test_accuracy_translation():
    """Translation (3.5, -2.25) at 64^2, 4 levels, defaults: the interior median end-point error (8 px margin) of the oracle
    is <= 0.1 px (0.023 when this was written) and the HIP estimate's is within the oracle's + 8 delta."""
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow
    I1, I2 = shifted_pair(0, 64, 64, 3.5, -2.25)
    (f64, b64), (f32, b32) = est_ref((64, 64, 4), I1, I2, levels=4)
    delta = float(max((f32.double() - f64).abs().max(), (b32.double() - b64).abs().max()))
    assert delta < DELTA_MAX
    fwd, bwd = PyramidLKFlow()(I1.float().cuda(), I2.float().cuda())                 # default levels at 64^2 = 4
    inner = (slice(8, -8), slice(8, -8))
    for name, got, ref, want in (("fwd", fwd, f64, (3.5, -2.25)), ("bwd", bwd, b64, (-3.5, 2.25))):
        e_ref, e_hip = fo.median_epe(ref[0], want, inner), fo.median_epe(got[0].double().cpu(), want, inner)
        print(f"[flowest translation {name}] median EPE oracle {e_ref:.4f} hip {e_hip:.4f} px")
        assert e_ref <= 0.1 and e_hip <= e_ref + FACTOR * delta


def test_accuracy_moving_patch():
    """A 24 x 24 patch at (16, 20) moving by (5, -3) over a static background, 64^2, defaults: forward flow inside the patch
    (4 px margin) median error <= 0.25 px, background away from the patch <= 0.05 px; the backward flow, on the moved patch
    with the sign flipped, is held to the same bounds."""
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow
    I1, I2 = (rep(x) for x in fo.patch_pair())
    fwd, bwd = PyramidLKFlow()(I1.float().cuda(), I2.float().cuda())
    fwd, bwd = fwd[0].double().cpu(), bwd[0].double().cpu()
    away = (slice(52, 64), slice(0, 64))
    e = {"fwd patch": fo.median_epe(fwd, (5, -3), (slice(20, 36), slice(24, 40))),
         "bwd patch": fo.median_epe(bwd, (-5, 3), (slice(25, 41), slice(21, 37))),
         "fwd background": fo.median_epe(fwd, (0, 0), away), "bwd background": fo.median_epe(bwd, (0, 0), away)}
    print("[flowest moving patch]", {k: round(v, 4) for k, v in e.items()})
    assert e["fwd patch"] <= 0.25 and e["bwd patch"] <= 0.25
    assert e["fwd background"] <= 0.05 and e["bwd background"] <= 0.05


def test_two_calls_are_bit_identical():
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow
    I1, I2 = (x.float().cuda() for x in shifted_pair(2, 64, 64, -2.5, 1.75))
    flow = PyramidLKFlow()
    a = flow(I1, I2)
    b = flow(I1, I2)                                            # the cached workspace, fresh outputs
    c = PyramidLKFlow()(I1.clone(), I2.clone())                 # another instance
    assert a[0].data_ptr() != b[0].data_ptr()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z) and float(x.abs().max()) > 1.0
    # bf16 images are converted by the first launch: the same as converting them first
    d = flow(I1.bfloat16(), I2.bfloat16())
    e = flow(I1.bfloat16().float(), I2.bfloat16().float())
    assert torch.equal(d[0], e[0]) and torch.equal(d[1], e[1])


def test_graph_replay_on_new_images():
    """One captured call (kernel launches only, no host synchronisation) replays on new image contents and equals the eager
    call bit for bit."""
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow
    flow = PyramidLKFlow()
    first = [x.float().cuda() for x in shifted_pair(3, 64, 64, 1.0, 2.0)]
    s1, s2 = first[0].clone(), first[1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flow(s1, s2)                                            # allocates the cached workspace outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fwd, bwd = flow(s1, s2)
    for seed, shift in ((3, (1.0, 2.0)), (4, (-3.0, 0.5)), (5, (2.25, -3.5))):
        I1, I2 = (x.float().cuda() for x in shifted_pair(seed, 64, 64, *shift))
        s1.copy_(I1)
        s2.copy_(I2)
        g.replay()
        torch.cuda.synchronize()
        rf, rb = fwd.clone(), bwd.clone()
        ef, eb = PyramidLKFlow()(I1, I2)
        assert torch.equal(rf, ef) and torch.equal(rb, eb), seed
        assert fo.median_epe(rf[0].double().cpu(), shift, (slice(8, -8), slice(8, -8))) <= 0.1


# ------------------------------------------------------------------------------------------------- predict_flow, pipeline
def test_predict_flow_convention_and_masks():
    from afldm_amd.shift_utils import flow_estimation as fe, flow_utils as fu
    I1, I2 = (x.float().cuda() for x in shifted_pair(6, 64, 64, 3.0, -2.0))
    model = fe.PyramidLKFlow()
    fwd_flow, fwd_occ, bwd_flow, bwd_occ = fe.predict_flow(model, I1, I2)
    fwd, bwd = model(I1, I2)
    assert fwd_flow.shape == bwd_flow.shape == (1, 2, 64, 64) and fwd_occ.shape == bwd_occ.shape == (1, 1, 64, 64)
    assert torch.equal(fwd_flow, torch.flip(fwd, (1,))) and torch.equal(bwd_flow, torch.flip(bwd, (1,)))
    inner = fwd_flow[0, :, 8:-8, 8:-8]
    assert abs(float(inner[0].median()) - (-2.0)) <= 0.1 and abs(float(inner[1].median()) - 3.0) <= 0.1      # channel 0 = x
    wf, wb = fu.forward_backward_consistency_check(fwd_flow, bwd_flow)
    assert torch.equal(fwd_occ, wf) and torch.equal(bwd_occ, wb)
    assert set(fwd_occ.unique().tolist()) <= {0.0, 1.0}
    with pytest.raises(ValueError):
        fe.predict_flow(model, torch.cat([I1, I1]), torch.cat([I2, I2]))


@pytest.mark.parametrize("method", [0, 1, 2])
def test_pipeline_estimates_its_flows(method):
    """flow_model=PyramidLKFlow(): pipe(img1, img2, warp_method=m) equals the same seeded call with flows= from predict_flow
    on the pipeline's preprocessed images, within the rel-RMS 1e-4 test_gpu_flow.py holds two runs of the splat to (its atomic
    sums arrive in another order); without flow_model the call still raises."""
    from test_gpu_interp import _images, _tiny_pipeline, rel_rms
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow, predict_flow
    pipe, _ = _tiny_pipeline(torch.float32)
    images = _images(128)
    kw = dict(num_frames=5, num_inference_steps=4, output_type="latent", warp_method=method)
    with pytest.raises(NotImplementedError, match="GMFlow"):
        pipe(*images, **kw)
    assert pipe.flow_model is None
    size = pipe.unet.config.sample_size * pipe.vae_scale_factor
    fwd_flow, _, bwd_flow, _ = predict_flow(PyramidLKFlow(), *(pipe._image(im, size).cuda() for im in images))
    assert fwd_flow.shape == (1, 2, size, size) and float(fwd_flow.abs().max()) > 0.1
    want = pipe(*images, flows=(fwd_flow, bwd_flow), generator=torch.Generator().manual_seed(9), **kw)
    from afldm_amd.pipelines.image_interpolation_pipeline import LDMInterpolationPipeline
    pipe = LDMInterpolationPipeline(**pipe.components, flow_model=PyramidLKFlow())
    pipe.set_progress_bar_config(disable=True)
    timings = {}
    got = pipe(*images, generator=torch.Generator().manual_seed(9), timings=timings, **kw)
    r = rel_rms(got, want)
    print(f"[flowest pipeline method {method}] estimated vs supplied flows: rel-RMS {r:.2e}; flow_s {timings['flow_s']:.4f}")
    assert r <= 1e-4
    base = pipe(*images, **dict(kw, warp_method=3))             # warp_method 3 never estimates
    assert rel_rms(got[1:-1], base[1:-1]) > 1e-3                # the estimated flow moved the intermediate frames
