"""CPU tests of the image-interpolation surface: the slerp against a float64 restatement of the reference formula
(image_interpolation_pipeline.py:68-108), the two alpha vectors, argument validation, the script's options and the C ABI of
afldm_attention_interp."""
import importlib.util
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slerp64(p0, p1, t):
    a, b = p0.double().flatten().numpy(), p1.double().flatten().numpy()
    dot = float(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1 + 1e-7, 1 - 1e-7))
    th = math.acos(dot)
    return torch.from_numpy((a * math.sin(th - th * t) / math.sin(th) + b * math.sin(th * t) / math.sin(th))).view(p0.shape)


@pytest.mark.parametrize("t", [0.0, 0.25, 0.5, 1.0])
def test_slerp_matches_the_float64_formula(t):
    from afldm_amd.pipelines.image_interpolation_pipeline import slerp
    g = torch.Generator().manual_seed(4)
    p0, p1 = torch.randn(4, 32, 32, generator=g), torch.randn(4, 32, 32, generator=g)
    for q1 in (p1, -p0 * 0.5, p0 * 3.0, p0 + 1e-6 * p1):           # generic, antiparallel, parallel, near-parallel (clamped)
        got = slerp(p0, q1, t)
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        want = _slerp64(p0, q1, t).float()
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)
    assert slerp(p0.half(), p1.half(), t).dtype == torch.float16
    assert slerp(p0.to(torch.bfloat16), p1.to(torch.bfloat16), t).dtype == torch.float32


def test_slerp_endpoints():
    from afldm_amd.pipelines.image_interpolation_pipeline import slerp
    g = torch.Generator().manual_seed(5)
    p0, p1 = torch.randn(2, 8, 8, generator=g), torch.randn(2, 8, 8, generator=g)
    assert torch.allclose(slerp(p0, p1, 0.0), p0, atol=1e-6) and torch.allclose(slerp(p0, p1, 1.0), p1, atol=1e-6)


def test_alpha_vectors():
    from afldm_amd.pipelines.image_interpolation_pipeline import interp_alphas
    fr, w = interp_alphas(17)
    assert len(fr) == len(w) == 17 and fr[0] == w[0] == 0.0 and fr[-1] == w[-1] == 1.0
    assert fr == [float(a) for a in torch.linspace(0, 1, 17)] and w == [f / 16 for f in range(17)]
    fr7, w7 = interp_alphas(7)
    assert fr7[1] == float(torch.tensor(1 / 6, dtype=torch.float32)) != w7[1] == 1 / 6   # fp32 linspace vs the Python f / (n - 1)
    assert interp_alphas(2) == ([0.0, 1.0], [0.0, 1.0])


def test_argument_validation():
    from afldm_amd.pipelines.image_interpolation_pipeline import check_interp_args
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    ddim = ffhq_ddim_scheduler()
    check_interp_args(ddim, 2, 3)
    for wm in (0, 1, 2):
        with pytest.raises(NotImplementedError, match="GMFlow"):
            check_interp_args(ddim, 17, wm)
    for n in (1, 0, 2.5):
        with pytest.raises(ValueError, match="num_frames"):
            check_interp_args(ddim, n, 3)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        check_interp_args(DPMSolverMultistepScheduler.from_config(ddim.config), 17, 3)


def test_attn_state_alpha_and_pair_slot():
    from afldm_amd.pipelines.cross_frame_attn import AttnState, CrossFrameAttnProcessor
    st = AttnState()
    st.set_alpha(0.3)
    assert st.alpha == 0.3
    v = torch.tensor([0.0, 0.5, 1.0])
    st.set_alpha(v)
    assert st.alpha is v
    with pytest.raises(ValueError):
        st.set_alpha(torch.zeros(2, 2))
    with pytest.raises(ValueError):
        st.set_alpha(torch.zeros(3, dtype=torch.float64))
    st.set_store_id(AttnState.PAIR)
    assert st.store_id == AttnState.PAIR not in (0, 1)
    assert CrossFrameAttnProcessor(st, enable_interp=True, cache_kv=True).cache_kv


def _script():
    spec = importlib.util.spec_from_file_location("image_interpolation_ffhq", os.path.join(ROOT, "scripts", "image_interpolation_ffhq.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options():
    s = _script()
    a = s.parse_args(["--random-init"])
    assert (a.n_frames, a.n_steps, a.output_path, a.dtype, a.eager, a.input_path_1) == (17, 50, "results/interp.gif", "fp32", False, None)
    a = s.parse_args(["--input_path_1", "a.png", "--input_path_2", "b.png", "--n_frames", "5", "--n_steps", "10", "--eager",
                      "--dtype", "bf16", "--seed", "3", "--ckpt", "/x", "--output_path", "o.gif"])
    assert (a.input_path_1, a.input_path_2, a.n_frames, a.n_steps, a.eager, a.dtype, a.seed, a.ckpt, a.output_path) == \
        ("a.png", "b.png", 5, 10, True, "bf16", 3, "/x", "o.gif")
    for bad in (["--random-init", "--n_frames", "1"], ["--input_path_1", "a.png"]):
        with pytest.raises(SystemExit):
            s.parse_args(bad)
    im = s.synthetic_images(7, size=64)
    assert len(im) == 2 and im[0].shape == (1, 3, 64, 64) and float(im[0].abs().max()) <= 1.0 and not torch.equal(im[0], im[1])


def test_attention_interp_is_declared_and_exported():
    from afldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    assert re.search(r"int afldm_attention_interp\(const void\* q, int ldq, const void\* k0, const void\* k1, int ldk,", hdr)
    assert "afldm_attention_interp" in _lib.EXPORTS and hasattr(_lib.lib, "afldm_attention_interp")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T afldm_attention_interp$", nm, re.M)
    assert "afldm_attention_interp" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
