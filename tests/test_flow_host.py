"""CPU tests of the flow-warping surface: the vectorised splat oracle (tests/flow_oracle.py) against the reference's recorded
outputs, argument validation of the pipeline's `flows`, the alias import, the C ABI of afldm_flow_splat / afldm_flow_warp and
the refusal of CPU tensors."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flow_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g17_flow.npz")


@pytest.mark.parametrize("name", ["rand32", "neg64"])
def test_oracle_matches_the_recorded_reference(name):
    """occ equal; res within the reorder bound (k + 1) 2^-23 mag: the reference sums the same fp32 terms in fp32, in source
    order, the oracle in float64."""
    z = np.load(GOLDEN)
    o = fo.splat(z[f"splat_{name}_x"][0], z[f"splat_{name}_flow"][0])
    assert not o["ambiguous"].any()
    assert np.array_equal(o["occ"], z[f"splat_{name}_occ"][0, 0] > 0.5)
    err = np.abs(o["res"] - z[f"splat_{name}_res"][0])
    assert np.all(err <= o["bound"]), float((err / np.maximum(o["bound"], 1e-300)).max())
    assert 0.01 < o["occ"].mean() < 0.2
    assert (o["cnt"] < 0).mean() > 0.005          # sources cross the top / left border: targets that end with cnt < 0


def test_oracle_pick_and_pool():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 16, 16)).astype(np.float32)
    flow = np.zeros((2, 16, 16), dtype=np.float32)
    o = fo.splat(x, flow)                                         # zero flow: the identity, one contribution of coefficient 1
    assert np.array_equal(o["res"], x.astype(np.float64)) and not o["occ"].any() and np.all(o["k"] == 1)
    flow[0] = 16.0                                                # everything leaves: all occluded, nothing lands
    o = fo.splat(x, flow)
    assert o["occ"].all() and not o["k"].any() and not o["ambiguous"].any()
    fill = rng.standard_normal((2, 16, 16))
    res, bound, occ, _ = fo.pick(o, 8, fill)
    assert np.array_equal(res, fill[:, ::8, ::8]) and not bound.any() and occ.all()
    pooled, pb = fo.pool(o, 8, fill)
    assert np.allclose(pooled, fill.reshape(2, 2, 8, 2, 8).sum(axis=(2, 4)) / 8) and np.all(pb > 0)
    # integer landing points hand their second neighbours an exact zero: not a contribution
    flow[0] = 3.0
    o = fo.splat(x, flow)
    assert np.all(o["k"][3:] == 1) and not o["k"][:3].any() and not o["ambiguous"].any()
    assert np.array_equal(o["res"][:, 3:], x[:, :-3].astype(np.float64))


def test_flow_argument_validation():
    from afldm_amd.pipelines.image_interpolation_pipeline import check_interp_args
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    ddim = ffhq_ddim_scheduler()
    f = torch.zeros(1, 2, 128, 128)
    for wm in (0, 1, 2, 3):
        check_interp_args(ddim, 5, wm, (f, f), 128)
        check_interp_args(ddim, 5, wm, [f, f])
    check_interp_args(ddim, 2, 3)                                # the three-argument form
    for wm in (0, 1, 2):
        with pytest.raises(NotImplementedError, match="GMFlow"):
            check_interp_args(ddim, 17, wm)
        with pytest.raises(NotImplementedError, match="GMFlow"):
            check_interp_args(ddim, 17, wm, None, 128)
    for bad in ((f,), (f, f, f), f, "fwd"):
        with pytest.raises(ValueError, match="pair"):
            check_interp_args(ddim, 5, 0, bad, 128)
    for bad in (torch.zeros(1, 2, 64, 64), torch.zeros(2, 128, 128), torch.zeros(1, 3, 128, 128), torch.zeros(2, 2, 128, 128),
                torch.zeros(1, 2, 128, 64), np.zeros((1, 2, 128, 128))):
        with pytest.raises(ValueError, match="fwd_flow"):
            check_interp_args(ddim, 5, 0, (bad, f), 128)
        with pytest.raises(ValueError, match="bwd_flow"):
            check_interp_args(ddim, 5, 1, (f, bad), 128)
    with pytest.raises(ValueError, match="warp_method"):
        check_interp_args(ddim, 5, 4, (f, f), 128)
    with pytest.raises(ValueError, match="num_frames"):
        check_interp_args(ddim, 1, 0, (f, f), 128)


def test_alias_import_and_surface():
    import afldm  # noqa: F401
    import afldm.shift_utils.flow_utils as alias
    import afldm_amd.shift_utils.flow_utils as fu
    assert alias is fu
    for name in ("coords_grid", "bilinear_sample", "flow_warp", "flow_warp_with_occ_bg", "forward_flow_warp",
                 "forward_upsample_flow_warp", "forward_backward_consistency_check", "get_patch_moving_flow", "upsample_noise",
                 "collect_noise_pixel", "continuous_noise_fwd_warp", "forward_flow_warp_frames"):
        assert callable(getattr(fu, name)), name
    for name in ("predict_flow", "get_warped_and_mask", "alpha_warp", "InputPadder", "flow_warp2", "flow_revserse_map",
                 "get_intermediate_warp_mask", "continuous_noise_warp", "continuous_noise_warp_bwd", "image_random_translate"):
        assert not hasattr(fu, name), name                      # out of scope: absent, not stubbed
    g = fu.coords_grid(2, 3, 4)
    assert g.shape == (2, 2, 3, 4) and g[0, 0, 1, 2] == 2 and g[0, 1, 1, 2] == 1          # channel 0 = x
    assert fu.coords_grid(1, 3, 4, homogeneous=True).shape == (1, 3, 3, 4)
    src = open(fu.__file__).read()
    assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S)


def test_cpu_tensors_are_refused():
    from afldm_amd import ops
    from afldm_amd.shift_utils import flow_utils as fu
    x, flow = torch.zeros(1, 2, 16, 16), torch.zeros(1, 2, 16, 16)
    for call in (lambda: fu.forward_flow_warp(x, flow), lambda: fu.flow_warp(x, flow), lambda: fu.bilinear_sample(x, flow),
                 lambda: fu.forward_upsample_flow_warp(x, torch.zeros(1, 2, 128, 128)),
                 lambda: fu.forward_flow_warp_frames(x, flow, [0.5]), lambda: fu.continuous_noise_fwd_warp(x, flow, 0.5, 8),
                 lambda: fu.upsample_noise(x, 8), lambda: fu.collect_noise_pixel(x, torch.zeros(1, 1, 16, 16), 8),
                 lambda: fu.flow_warp_with_occ_bg(x, flow, torch.ones(1, 1, 16, 16), True),
                 lambda: fu.forward_backward_consistency_check(flow, flow),
                 lambda: ops.flow_splat(x, flow, torch.ones(1)), lambda: ops.flow_warp(x, flow)):
        with pytest.raises(RuntimeError, match="cuda|no CPU path"):
            call()


def test_flow_entry_points_are_declared_and_exported():
    from afldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    assert re.search(r"int afldm_flow_splat\(const void\* x, const float\* flow, const float\* scale, const void\* fill,", hdr)
    assert re.search(r"size_t afldm_flow_splat_workspace\(int B, int C, int H, int W, int ds, int mode\);", hdr)
    assert re.search(r"int afldm_flow_warp\(const void\* x, const float\* flow, void\* y, unsigned char\* mask,", hdr)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("afldm_flow_splat", "afldm_flow_splat_workspace", "afldm_flow_warp"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert re.search(rf" T {name}$", nm, re.M) and name in doc
    # the workspace size is host arithmetic: pick keeps H/ds x W/ds targets, pool the whole plane; bad arguments give 0
    ws = _lib.lib.afldm_flow_splat_workspace
    assert ws(15, 4, 256, 256, 8, 0) == 15 * 5 * 32 * 32 * 4 and ws(15, 4, 256, 256, 8, 1) == 15 * 5 * 256 * 256 * 4
    assert ws(1, 4, 30, 32, 8, 0) == 0 and ws(1, 4, 32, 32, 8, 2) == 0 and ws(0, 4, 32, 32, 8, 0) == 0
    src = open(os.path.join(ROOT, "afldm_amd", "csrc", "flow.hip")).read()
    assert "flow.hip" in open(os.path.join(ROOT, "afldm_amd", "build.py")).read()
    assert "flow_utils_np.py:116-152" in src and "flow_utils.py:53-86" in src          # each entry cites what it replaces


def test_script_flow_options(tmp_path):
    spec = importlib.util.spec_from_file_location("image_interpolation_ffhq", os.path.join(ROOT, "scripts", "image_interpolation_ffhq.py"))
    s = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(s)
    a = s.parse_args(["--random-init"])
    assert a.warp_method == 3 and a.flow is None
    a = s.parse_args(["--random-init", "--warp-method", "0", "--flow", "f.npz"])
    assert a.warp_method == 0 and a.flow == "f.npz"
    for bad in (["--random-init", "--warp-method", "1"], ["--random-init", "--warp-method", "4", "--flow", "f.npz"]):
        with pytest.raises(SystemExit):
            s.parse_args(bad)
    path = str(tmp_path / "f.npz")
    np.savez(path, fwd=np.ones((2, 8, 8), dtype=np.float64), bwd=np.zeros((1, 2, 8, 8), dtype=np.float32))
    fwd, bwd = s.load_flows(path)
    assert fwd.shape == bwd.shape == (1, 2, 8, 8) and fwd.dtype == torch.float32 and float(fwd.mean()) == 1.0
    np.savez(path, fwd=np.ones((2, 8, 8)))
    with pytest.raises(SystemExit):
        s.load_flows(path)
