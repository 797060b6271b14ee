"""CPU tests of the built-in flow estimator's surface: the oracle's accuracy cases in fp64 (tests/flowest_oracle.py),
argument validation, the refusal of CPU tensors, the alias import, the C ABI of the afldm_flowest_* entry points, and that
everything existing stays as it was: flow_utils gains no name and a pipeline built without flow_model keeps raising."""
import importlib.util
import os
import re
import subprocess

import pytest
import torch

import flowest_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("afldm_flowest_pyr_down", "afldm_flowest_up2", "afldm_flowest_lk_step", "afldm_flowest_smooth")


def test_oracle_accuracy_translation():
    """Translation (3.5, -2.25) at 64^2, 4 levels (the default there), defaults: interior median end-point error, 8 px margin,
    <= 0.1 px (0.023 forward when this was written)."""
    I1 = fo.texture(0, 64)
    I2 = fo.translate(I1, 3.5, -2.25)
    assert fo.default_levels(64, 64) == 4
    fwd, bwd = fo.bidirectional(I1, I2)
    inner = (slice(8, -8), slice(8, -8))
    ef, eb = fo.median_epe(fwd[0], (3.5, -2.25), inner), fo.median_epe(bwd[0], (-3.5, 2.25), inner)
    print(f"[flowest oracle translation] median EPE fwd {ef:.4f} bwd {eb:.4f} px")
    assert ef <= 0.1 and eb <= 0.1
    f32, b32 = fo.bidirectional(I1.float(), I2.float())          # the fp32 run stays next to the fp64 run
    assert float((f32.double() - fwd).abs().max()) < 1e-3 and float((b32.double() - bwd).abs().max()) < 1e-3


def test_oracle_accuracy_moving_patch():
    """A 24 x 24 patch at (16, 20) moving by (5, -3) over a static background at 64^2: <= 0.25 px inside the patch (4 px
    margin), <= 0.05 px on the background away from it; the backward flow the same with the sign flipped."""
    I1, I2 = fo.patch_pair()
    assert torch.equal(I1[..., 16:40, 20:44], I2[..., 21:45, 17:41]) and torch.equal(I1[..., 52:, :], I2[..., 52:, :])
    fwd, bwd = fo.bidirectional(I1, I2)
    away = (slice(52, 64), slice(0, 64))
    assert fo.median_epe(fwd[0], (5, -3), (slice(20, 36), slice(24, 40))) <= 0.25
    assert fo.median_epe(bwd[0], (-5, 3), (slice(25, 41), slice(21, 37))) <= 0.25
    assert fo.median_epe(fwd[0], (0, 0), away) <= 0.05 and fo.median_epe(bwd[0], (0, 0), away) <= 0.05


def test_oracle_pieces():
    x = fo.texture(1, 16, 2, 24)
    assert x.shape == (1, 2, 16, 24) and float(x.abs().max()) == 1.0
    assert fo.pyr_down(x).shape == (1, 2, 8, 12)
    one = torch.ones(1, 2, 8, 12, dtype=torch.float64)
    assert torch.equal(fo.pyr_down(one), torch.ones(1, 2, 4, 6, dtype=torch.float64))
    assert torch.equal(fo.smooth(one), one) and torch.equal(fo.up2(one), 2 * torch.ones(1, 2, 16, 24, dtype=torch.float64))
    # an interior pixel of pyr_down: rows 2y-1 .. 2y+2, columns 2x-1 .. 2x+2 under [1, 3, 3, 1] / 8
    w = torch.tensor([1., 3., 3., 1.], dtype=torch.float64) / 8
    want = (w[:, None] * w[None, :] * x[0, 0, 3:7, 5:9]).sum()
    assert abs(float(fo.pyr_down(x)[0, 0, 2, 3] - want)) < 1e-15
    # zero flow on identical images stays zero; the step is clamped to one pixel
    z = torch.zeros(1, 2, 16, 24, dtype=torch.float64)
    assert torch.equal(fo.lk_step(x, x, z), z)
    step = fo.lk_step(x, fo.translate(x, 6.0, -5.0), z)
    assert float(step.norm(dim=1).max()) <= 1.0 + 1e-12
    with pytest.raises(ValueError):
        fo.estimate(x, x, levels=5)                              # 24 is not divisible by 16


def test_argument_validation():
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow, default_levels
    assert default_levels(256, 256) == 6 and default_levels(64, 32) == 3
    for bad in (dict(radius=0), dict(radius=-1), dict(radius=5), dict(levels=0), dict(levels=-2), dict(iters=0), dict(lam=0.0),
                dict(radius=2.5)):
        with pytest.raises(ValueError):
            PyramidLKFlow(**bad)
    flow = PyramidLKFlow(levels=4)
    ok = torch.zeros(1, 3, 64, 64)
    for a, b in ((torch.zeros(1, 3, 60, 64), torch.zeros(1, 3, 60, 64)),          # 60 is not divisible by 2^3
                 (torch.zeros(1, 3, 64, 36), torch.zeros(1, 3, 64, 36)),
                 (torch.zeros(1, 5, 64, 64), torch.zeros(1, 5, 64, 64)),          # C > 4
                 (ok, torch.zeros(1, 3, 32, 32)), (ok, ok.double()), (ok[0], ok[0])):
        with pytest.raises(ValueError):
            flow(a, b)
    with pytest.raises(ValueError, match="divisible"):
        PyramidLKFlow()(torch.zeros(1, 3, 42, 40), torch.zeros(1, 3, 42, 40))     # default levels 3: 42 is not divisible by 4


def test_cpu_tensors_are_refused():
    from afldm_amd import ops
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow, predict_flow
    x, u = torch.zeros(1, 3, 64, 64), torch.zeros(1, 2, 64, 64)
    for call in (lambda: PyramidLKFlow()(x, x), lambda: PyramidLKFlow(levels=1)(x.bfloat16(), x.bfloat16()),
                 lambda: predict_flow(PyramidLKFlow(), x, x), lambda: ops.flowest_pyr_down(x), lambda: ops.flowest_pyr_down(x, factor=1),
                 lambda: ops.flowest_up2(u), lambda: ops.flowest_smooth(u), lambda: ops.flowest_lk_step(x, x, u)):
        with pytest.raises(RuntimeError, match="cuda|no CPU path"):
            call()


def test_predict_flow_checks_both_images():
    from afldm_amd.shift_utils.flow_estimation import predict_flow

    def model(a, b):
        raise AssertionError("the estimator must not be reached")

    ok = torch.zeros(1, 3, 64, 64)
    for a, b in ((torch.zeros(2, 3, 64, 64), ok), (ok, torch.zeros(2, 3, 64, 64)), (ok, torch.zeros(1, 3, 32, 32)), (ok, ok[0]),
                 (ok, None)):
        with pytest.raises(ValueError, match="image"):
            predict_flow(model, a, b)


def test_alias_import_and_surface():
    import afldm  # noqa: F401
    import afldm.shift_utils.flow_estimation as alias
    import afldm_amd.shift_utils.flow_estimation as fe
    import afldm_amd.shift_utils.flow_utils as fu
    assert alias is fe
    assert callable(fe.PyramidLKFlow) and callable(fe.predict_flow)
    for name in ("get_warped_and_mask", "alpha_warp", "InputPadder"):          # need flow_warp2 / GMFlow's padding: absent
        assert not hasattr(fe, name), name
    for name in ("predict_flow", "get_warped_and_mask", "alpha_warp", "InputPadder", "PyramidLKFlow"):
        assert not hasattr(fu, name), name                      # the estimator lives in its own module
    src = open(fe.__file__).read()
    assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S)
    assert "GMFlow" in fe.__doc__ and "NOT GMFlow" in fe.__doc__               # says plainly what it is not


def test_pipeline_without_flow_model_keeps_raising():
    """The pipeline refuses before any work, so tiny CPU stand-ins for the models are enough."""
    import inspect
    from afldm_amd.pipelines.image_interpolation_pipeline import LDMInterpolationPipeline, check_interp_args
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    assert list(inspect.signature(LDMInterpolationPipeline.__init__).parameters) == ["self", "vae", "unet", "scheduler", "flow_model"]
    assert inspect.signature(LDMInterpolationPipeline.__init__).parameters["flow_model"].default is None

    class Cfg:
        sample_size, block_out_channels = 16, [1, 1, 1, 1]

    class Stub(torch.nn.Module):
        config, device = Cfg(), torch.device("cpu")

    pipe = LDMInterpolationPipeline(Stub(), Stub(), ffhq_ddim_scheduler())
    assert pipe.flow_model is None and sorted(pipe.components) == ["scheduler", "unet", "vae"]
    img = torch.zeros(1, 3, 128, 128)
    for wm in (0, 1, 2):
        with pytest.raises(NotImplementedError, match="GMFlow"):
            pipe(img, img, warp_method=wm)
        with pytest.raises(NotImplementedError, match="GMFlow"):
            check_interp_args(pipe.scheduler, 17, wm)
    # with a flow_model the flows come from predict_flow on the two preprocessed images, before check_interp_args
    seen = []

    def model(a, b):
        seen.append((tuple(a.shape), tuple(b.shape)))
        raise RuntimeError("reached the estimator")

    pipe = LDMInterpolationPipeline(Stub(), Stub(), ffhq_ddim_scheduler(), flow_model=model)
    with pytest.raises(RuntimeError, match="reached the estimator"):
        pipe(torch.zeros(1, 3, 64, 64), img, warp_method=0)
    assert seen == [((1, 3, 128, 128), (1, 3, 128, 128))]
    for bad in (dict(num_frames=1), dict(num_frames=2.5)):                      # refused before the estimator runs
        with pytest.raises(ValueError, match="num_frames"):
            pipe(img, img, warp_method=0, **bad)
    assert len(seen) == 1
    flows = (torch.zeros(1, 2, 64, 64), torch.zeros(1, 2, 128, 128))            # the caller's flows win, and are still checked
    with pytest.raises(ValueError, match="fwd_flow"):
        pipe(img, img, warp_method=0, flows=flows)
    assert len(seen) == 1


def test_entry_points_are_declared_exported_and_documented():
    from afldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    assert re.search(r"int afldm_flowest_pyr_down\(const void\* x, float\* y, int n, int H, int W, int factor, int dtype, afldm_stream_t stream\);", hdr)
    assert re.search(r"int afldm_flowest_lk_step\(const float\* I1, const float\* I2, const float\* u_in, float\* u_out, int B, int C,", hdr)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert re.search(rf" T {name}$", nm, re.M) and name in doc and name in hdr
    build = open(os.path.join(ROOT, "afldm_amd", "build.py")).read()
    src = open(os.path.join(ROOT, "afldm_amd", "csrc", "flowest.hip")).read()
    assert "flowest.hip" in build and "#pragma clang fp contract(off)" in src and "atomic" not in src.replace("no atomic", "")
    # host-side refusals of the C ABI need no device: NULL pointers and bad shapes return a status before any launch
    lib = _lib.lib
    assert lib.afldm_flowest_pyr_down(None, None, 1, 16, 16, 2, 0, None) != 0
    assert lib.afldm_flowest_lk_step(None, None, None, None, 1, 3, 16, 16, 3, 1e-3, 0, None) != 0
    assert lib.afldm_flowest_smooth(None, None, 1, 16, 16, None) != 0 and lib.afldm_flowest_up2(None, None, 1, 8, 8, None) != 0
    assert b"afldm_flowest_up2" in lib.afldm_last_error()


def test_script_flow_estimate_option(tmp_path):
    spec = importlib.util.spec_from_file_location("image_interpolation_ffhq", os.path.join(ROOT, "scripts", "image_interpolation_ffhq.py"))
    s = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(s)
    a = s.parse_args(["--random-init", "--warp-method", "0", "--flow", "estimate"])
    assert a.warp_method == 0 and a.flow == "estimate"
    assert s.parse_args(["--random-init", "--warp-method", "2", "--flow", "f.npz"]).flow == "f.npz"
    with pytest.raises(SystemExit):
        s.parse_args(["--random-init", "--warp-method", "1"])
    # `estimate` hands the pipeline the built-in estimator and passes no flows; a file leaves the pipeline as it is
    import types
    import numpy as np
    from afldm_amd.shift_utils.flow_estimation import PyramidLKFlow
    pipe = types.SimpleNamespace(flow_model=None)
    assert s.flow_source(pipe, "estimate") is None and isinstance(pipe.flow_model, PyramidLKFlow)
    pipe = types.SimpleNamespace(flow_model=None)
    assert s.flow_source(pipe, None) is None and pipe.flow_model is None
    path = str(tmp_path / "f.npz")
    np.savez(path, fwd=np.ones((2, 8, 8), dtype=np.float32), bwd=np.zeros((2, 8, 8), dtype=np.float32))
    fwd, bwd = s.flow_source(pipe, path)
    assert fwd.shape == bwd.shape == (1, 2, 8, 8) and pipe.flow_model is None
