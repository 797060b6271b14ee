"""CPU tests of the frame-sequence editing surface: the keyframe source table against the formula restated in
tests/video_oracle.py, the truncated inversion rows against the reference's lines restated there, AttnState's new fields, the C ABI
of afldm_attention_bank, the script's options and the pipeline's signature."""
import importlib.util
import inspect
import itertools
import os
import re
import subprocess
import sys

import pytest
import torch

import video_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_keyframes(F):
    """every sorted tuple of distinct indices < F that begins with 0"""
    for n in range(F):
        for rest in itertools.combinations(range(1, F), n):
            yield (0,) + rest


def test_video_sources_matches_the_formula_for_every_small_case():
    from afldm_amd.pipelines.video_editing_pipeline import video_sources
    cases = 0
    for F in range(1, 10):
        for keys in _all_keyframes(F):
            src, alpha = video_sources(F, keys)
            want_src, want_alpha = vo.sources(F, keys)
            assert src.dtype == torch.int32 and tuple(src.shape) == (F, 2) and src.device.type == "cpu"
            assert alpha.dtype == torch.float32 and tuple(alpha.shape) == (F,)
            assert src.tolist() == [list(s) for s in want_src], (F, keys)
            assert torch.equal(alpha, torch.tensor(want_alpha, dtype=torch.float32)), (F, keys)
            for f in range(F):
                if f in keys or f > keys[-1]:
                    assert float(alpha[f]) == 0.0 and src[f, 0] == src[f, 1], (F, keys, f)      # exactly 0: the kernel's skip
                else:
                    assert 0.0 < float(alpha[f]) < 1.0 and src[f, 1] == src[f, 0] + 1, (F, keys, f)
                assert 0 <= int(src[f, 0]) <= int(src[f, 1]) < len(keys)
            cases += 1
    assert cases == sum(2 ** (F - 1) for F in range(1, 10))


def test_video_sources_single_keyframe_is_the_reference():
    from afldm_amd.pipelines.video_editing_pipeline import video_sources
    src, alpha = video_sources(6, (0,))
    assert src.tolist() == [[0, 0]] * 6 and alpha.tolist() == [0.0] * 6


@pytest.mark.parametrize("F,keys", [(5, (2, 0)), (5, (0, 2, 2)), (5, (1, 3)), (5, (0, 5)), (3, (0, 7)), (5, ()), (5, (0, 1.5)),
                                    (5, (0, -1)), (5, 3)])
def test_video_sources_refuses_bad_keyframes(F, keys):
    from afldm_amd.pipelines.video_editing_pipeline import video_sources
    assert not (isinstance(keys, tuple) and all(isinstance(k, int) for k in keys) and vo.valid_keyframes(F, keys))
    with pytest.raises(ValueError, match="keyframe"):
        video_sources(F, keys)


@pytest.mark.parametrize("strength", [-1, 0.3, 0.7, 1.0])
@pytest.mark.parametrize("steps", [7, 50])
def test_inversion_rows_over_the_truncated_timesteps(strength, steps):
    from afldm_amd.pipelines.video_editing_pipeline import inversion_rows, video_timesteps
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    sch = ffhq_ddim_scheduler()
    sch.set_timesteps(steps)
    everything = list(sch._timesteps_host)
    ts = video_timesteps(sch, steps, strength)
    want_ts = vo.get_timesteps(everything, steps, strength)
    assert ts == want_ts and len(ts) == (steps if strength < 0 else min(int(steps * strength), steps)) and len(ts) >= 1
    rows = inversion_rows(sch, ts)
    want = vo.inversion_rows(sch.alphas_cumprod, sch.final_alpha_cumprod, ts)
    assert [t for t, _ in rows] == [w[0] for w in want] == list(reversed(ts))
    for (t, got), w in zip(rows, want):
        assert got == pytest.approx(w[1:], rel=1e-6, abs=0), (t, got, w)
    # i == 0 of the truncated list takes final_alpha_cumprod, whatever timestep the truncation starts at
    assert rows[0][1][0] == pytest.approx(float(sch.final_alpha_cumprod) ** 0.5, rel=1e-6)
    # the pipeline's two schedules: these rows, and DDIMScheduler.step's coefficients of the kept timesteps
    from afldm_amd.pipelines.video_editing_pipeline import LDMVideoPipeline
    pipe = LDMVideoPipeline(None, _FakeUNet(), sch)
    fwd, inv = pipe._schedules(steps, strength)
    assert list(inv.timesteps) == [t for t, _ in rows] and list(fwd.timesteps) == ts
    assert [tuple(r) for r in inv.rows] == [tuple(float(v) for v in c) for _, c in rows]
    sch.set_timesteps(steps)
    assert [tuple(r) for r in fwd.rows] == [tuple(sch.coefficients(t)) for t in ts]


class _FakeUNet(torch.nn.Module):
    pass


def test_strength_outside_the_schedule_is_refused():
    from afldm_amd.pipelines.video_editing_pipeline import video_timesteps
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    for bad in (0.0, 0.01, 1.5):
        with pytest.raises(ValueError, match="strength"):
            video_timesteps(ffhq_ddim_scheduler(), 10, bad)


def test_attn_state_sources_and_bank_slot():
    from afldm_amd.pipelines.cross_frame_attn import AttnState, CrossFrameAttnProcessor
    st = AttnState()
    assert st.sources is None
    t = torch.tensor([[0, 1], [2, 2]], dtype=torch.int32)
    st.set_sources(t)
    assert st.sources is t
    with pytest.raises(AttributeError, match="read-only"):
        st.sources = t
    for bad in (torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32),
                [[0, 1]]):
        with pytest.raises(ValueError, match="int32"):
            st.set_sources(bad)
    assert AttnState.BANK not in (0, 1, AttnState.PAIR)
    st.set_store_id(AttnState.BANK)
    assert st.store_id == AttnState.BANK
    st.reset()
    assert st.sources is None and st.store_id == 0 and st.alpha == 0
    p = CrossFrameAttnProcessor(st, cache_kv=True, enable_bank=True)
    assert p.enable_bank and p.cache_kv and not p.enable_interp
    assert not CrossFrameAttnProcessor(st).enable_bank
    with pytest.raises(ValueError):
        CrossFrameAttnProcessor(st, enable_interp=True, enable_bank=True)


def test_attention_bank_is_declared_bound_and_exported():
    from ctypes import c_float, c_int, c_void_p
    from afldm_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    decl = re.search(r"int afldm_attention_bank\(([^;]*)\);", hdr)
    assert decl, "afldm_attention_bank is not declared in include/afldm_hip.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const void* q", "int ldq", "const void* k", "int ldk", "const void* vt", "const int* src",
                      "const float* alpha", "void* o", "int ldo", "int B", "int S", "int heads", "int Tq", "int Tk", "int d",
                      "float scale", "int dtype", "afldm_stream_t stream"]
    fn = _lib.lib.afldm_attention_bank
    vp, ip, fp = c_void_p, c_int, c_float
    assert fn.argtypes == [vp, ip, vp, ip, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, ip, fp, ip, vp] and fn.restype is c_int
    assert len(fn.argtypes) == len(params) and "afldm_attention_bank" in _lib.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T afldm_attention_bank$", nm, re.M)
    assert "afldm_attention_bank" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the kernel is a mode of k_attn in csrc/attn.hip: no new source, and the one that holds it is built
    assert "attn.hip" in build.SOURCES
    assert "afldm_attention_bank" in open(os.path.join(build.CSRC, "attn.hip")).read()


def test_attention_bank_has_no_cpu_path_and_checks_its_operands():
    from afldm_amd import ops
    q, k, vt = torch.zeros(2, 16, 48), torch.zeros(3, 16, 48), torch.zeros(3, 48, 16)
    src, alpha = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attention_bank(q, k, vt, src, alpha, 2)
    assert list(inspect.signature(ops.attention_bank).parameters)[:7] == ["q", "k_bank", "vt_bank", "src", "alpha", "heads", "scale"]
    assert inspect.signature(ops.attention_bank).parameters["scale"].default is None


def test_pipeline_signature_and_alias():
    import afldm.pipelines.video_editing_pipeline as alias
    from afldm_amd.pipelines import video_editing_pipeline as mod
    assert alias is mod
    sig = inspect.signature(mod.LDMVideoPipeline.__call__)
    want = [("frames", inspect.Parameter.empty), ("num_inference_steps", 50), ("strength", -1), ("use_sdedit", False),
            ("keyframes", (0,)), ("generator", None), ("frame_batch", 16), ("output_type", "pil"), ("return_dict", True),
            ("use_graph", True)]
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == want
    assert list(inspect.signature(mod.LDMVideoPipeline.__init__).parameters)[1:] == ["vae", "unet", "scheduler"]
    assert list(inspect.signature(mod.video_sources).parameters) == ["num_frames", "keyframes"]


def test_sampler_and_processor_signatures():
    from afldm_amd.harness import CrossFrameSampler
    from afldm_amd.models.blocks import AttnProcessor2_0
    from afldm_amd.pipelines.cross_frame_attn import CrossFrameAttnProcessor
    assert inspect.signature(CrossFrameSampler.__init__).parameters["bank"].default is False
    assert inspect.signature(CrossFrameAttnProcessor.__init__).parameters["enable_bank"].default is False
    assert inspect.signature(AttnProcessor2_0.__call__).parameters["src"].default is None
    assert {"src", "alpha"} <= set(inspect.signature(CrossFrameSampler.run).parameters)


def _script():
    spec = importlib.util.spec_from_file_location("video_editing_ffhq", os.path.join(ROOT, "scripts", "video_editing_ffhq.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options():
    s = _script()
    a = s.parse_args(["--random-init"])
    assert (a.n_frames, a.n_steps, a.strength, a.keyframes, a.frame_batch, a.sdedit, a.eager, a.timings, a.output_path) == \
        (16, 50, -1.0, (0,), 16, False, False, None, "results/video_edit.gif")
    a = s.parse_args(["--ckpt", "/x", "--input", "clip.gif", "--strength", "0.7", "--keyframes", "0,4,8", "--n-frames", "9",
                      "--timings", "t.json", "--sdedit", "--frame-batch", "4", "--eager", "--dtype", "bf16"])
    assert (a.input, a.strength, a.keyframes, a.n_frames, a.timings, a.sdedit, a.frame_batch, a.eager, a.dtype) == \
        ("clip.gif", 0.7, (0, 4, 8), 9, "t.json", True, 4, True, "bf16")
    for bad in ([], ["--ckpt", "/x"], ["--random-init", "--sdedit"], ["--random-init", "--n-frames", "0"],
                ["--random-init", "--keyframes", "0,a"], ["--random-init", "--frame-batch", "0"]):
        with pytest.raises(SystemExit):
            s.parse_args(bad)
    fr = s.synthetic_frames(3, 5, size=64)
    assert fr.shape == (5, 3, 64, 64) and float(fr.abs().max()) <= 1.0 and not torch.equal(fr[0], fr[4])


def test_script_reads_directories_and_gifs(tmp_path):
    from PIL import Image
    s = _script()
    frames = [Image.new("RGB", (20, 12), (40 * i, 10, 200 - 40 * i)) for i in range(4)]
    for i, f in enumerate(frames):
        f.save(tmp_path / f"f{i:02d}.png")
    got = s.load_frames(str(tmp_path), 3, 16)
    assert len(got) == 3 and all(g.size == (16, 16) and g.mode == "RGB" for g in got)
    assert got[1].getpixel((3, 3)) == (40, 10, 160)
    gif = tmp_path / "clip.gif"
    frames[0].save(gif, save_all=True, append_images=frames[1:], duration=40, loop=0)
    got = s.load_frames(str(gif), 8, 16)
    assert len(got) == 4 and all(g.size == (16, 16) and g.mode == "RGB" for g in got)


def test_script_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "video_editing_ffhq.py"), "--help"], capture_output=True,
                       text=True)
    assert r.returncode == 0
    for opt in ("--strength", "--keyframes", "--n-frames", "--timings", "--input"):
        assert opt in r.stdout, opt
