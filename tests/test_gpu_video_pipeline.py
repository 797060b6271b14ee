"""Frame-sequence editing (reference afldm/pipelines/video_equiv_editing_pipeline.py:331-748) on MI355X: the banked LOAD of
one attention block against the float64 restatement in tests/video_oracle.py, the cached path against the eager yardstick,
LDMVideoPipeline's graph path against its statement-by-statement eager loop, the single-keyframe case against the existing
non-bank CrossFrameSampler bit for bit, chunking, replay, evaluation counts and the refusals.  Tiny UNet and tiny AF-VAE
(the builders of test_gpu_r02 / test_gpu_vae), 3-5 frames, 3-4 steps."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import attention_oracle as ao
import video_oracle as vo

pytestmark = pytest.mark.gpu

GRAPH_BOUND = 1e-4          # the graph-path bound of test_gpu_interp.py (graph against eager, fp32), reused by test_gpu_flow.py


def rel_rms(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


_built = {}


def _pipeline(dtype, vae=True):
    """One LDMVideoPipeline per (dtype, with / without VAE), shared by the tests of this module (its captured graphs too)."""
    key = (dtype, vae)
    if key not in _built:
        from test_gpu_r02 import build_unet
        from test_gpu_vae import build_vae
        from afldm_amd.pipelines.video_editing_pipeline import LDMVideoPipeline
        from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
        unet, _, _ = build_unet("tiny", dtype)
        pipe = LDMVideoPipeline(build_vae(torch.float32)[0] if vae else None, unet, ffhq_ddim_scheduler())
        pipe.set_progress_bar_config(disable=True)
        _built[key] = pipe
    return _built[key]


def _frames(n, size=128, seed=11):
    """n smooth frames [n, 3, size, size] in [-1, 1]: one random colour field drifting towards another"""
    g = torch.Generator().manual_seed(seed)
    a, b = (torch.rand(1, 3, 8, 8, generator=g) * 2 - 1 for _ in range(2))
    fields = torch.cat([a + (b - a) * (f / max(n - 1, 1)) + 0.1 * torch.randn(1, 3, 8, 8, generator=g) for f in range(n)])
    return F.interpolate(fields, size=(size, size), mode="bicubic", align_corners=False).clamp(-1, 1)


def _gen(seed=3):
    return torch.Generator().manual_seed(seed)


def _samplers(pipe):
    return {w: next(iter(getattr(pipe, f"_xframe_bank_sampler_{w}").values())) for w in ("inv", "fwd")
            if f"_xframe_bank_sampler_{w}" in pipe.__dict__}


@contextlib.contextmanager
def _count_unet_calls(unet):
    calls, real = [], unet.forward

    def counted(x, *a, **k):
        calls.append(x.shape[0])
        return real(x, *a, **k)
    unet.forward = counted
    try:
        yield calls
    finally:
        del unet.forward


# ----------------------------------------------------------------------------------------------- processor level
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_banked_load_of_one_attention_block_vs_float64(dtype, monkeypatch):
    """STORE a bank of S = 3 maps with store_id BANK, then a LOAD batch of 5 samples with their own source pairs and weights:
    the cached path (one afldm_attention_bank launch) and the eager yardstick (per sample and source: GroupNorm + K / V projection
    of the stored map + afldm_attention, torch blend) against GroupNorm -> projection -> blended attention -> to_out + residual in
    float64 on the dtype-rounded inputs and weights, within attention_oracle.TOL."""
    from afldm_amd import ops
    from afldm_amd.models.blocks import Attention
    from afldm_amd.pipelines.cross_frame_attn import AttnState, CrossFrameAttnProcessor
    C, heads, groups, side, S, B, t = 64, 4, 8, 8, 3, 5, 321
    g = torch.Generator().manual_seed(5)
    attn = Attention(C, heads=heads, dim_head=C // heads, eps=1e-5, norm_num_groups=groups, residual_connection=True, bias=True)
    with torch.no_grad():
        for prm in attn.parameters():
            prm.copy_(ao.rnd(torch.randn(prm.shape, generator=g) * (0.3 if prm.ndim == 1 else C ** -0.5) + (prm.ndim == 1) * 1.0, dtype))
    sd = {k: v.clone() for k, v in attn.state_dict().items()}
    attn = attn.cuda().to(dtype)
    bank = ao.rnd(torch.randn(S, side, side, C, generator=g) * (0.5 + torch.rand(1, 1, 1, C, generator=g)), dtype)
    x = ao.rnd(torch.randn(B, side, side, C, generator=g), dtype)
    src = [(0, 1), (2, 0), (1, 1), (2, 1), (0, 2)]
    alpha = [0.37, 0.81, 0.15, 0.0, 0.0]
    want = vo.bank_load(x, bank, src, alpha, sd, heads, groups, 1e-5)
    calls = []
    real = ops.attention_bank
    monkeypatch.setattr(ops, "attention_bank", lambda *a, **k: calls.append(a[0].shape[0]) or real(*a, **k))
    got = {}
    for cached in (True, False):
        st = AttnState()
        proc = CrossFrameAttnProcessor(st, cache_kv=cached, enable_bank=True)
        attn.set_processor(proc)
        st.set_timestep(t)
        st.set_store_id(AttnState.BANK)
        attn(bank.to(device="cuda", dtype=dtype))
        assert proc.maps[0][t].shape[0] == S and (not cached or proc.kv[0][t][0].shape[0] == S)
        assert not proc.maps[1] and not proc.kv[1]
        st.to_load()
        st.set_sources(torch.tensor(src, dtype=torch.int32, device="cuda"))
        st.set_alpha(torch.tensor(alpha, dtype=torch.float32, device="cuda"))
        got[cached] = attn(x.to(device="cuda", dtype=dtype)).float().cpu()
        why, mx, rms = ao.within(got[cached], want, dtype)
        print(f"[video processor, {dtype}, {'cached' if cached else 'eager'}] vs float64: max/scale {mx:.3e} rel-RMS {rms:.3e}")
        assert why is None, why
    assert calls == [B]                          # the cached LOAD is ONE bank launch; the eager yardstick makes none
    why, mx, rms = ao.within(got[True], got[False].double(), dtype)
    print(f"[video processor, {dtype}] cached vs eager: max/scale {mx:.3e} rel-RMS {rms:.3e}")
    assert why is None, why
    with pytest.raises(ValueError, match="set_sources"):
        st.set_sources(None)
        attn(x.to(device="cuda", dtype=dtype))


# ----------------------------------------------------------------------------------------------- graph against eager
STARTS = [("inversion", (0,), -1), ("inversion", (0, 2, 4), 0.7), ("sdedit", (0,), 0.7), ("sdedit", (0, 2, 4), 0.7),
          ("inversion", (0, 2, 4), -1)]


@pytest.mark.parametrize("start,keyframes,strength", STARTS, ids=[f"{s}-k{len(k)}-s{st}" for s, k, st in STARTS])
def test_graph_path_vs_eager_loop(start, keyframes, strength):
    from afldm_amd.pipelines.cross_frame_attn import get_unet_attn_processors
    pipe = _pipeline(torch.float32)
    frames = _frames(5)
    before = get_unet_attn_processors(pipe.unet)
    kw = dict(num_inference_steps=4, strength=strength, use_sdedit=start == "sdedit", keyframes=keyframes, output_type="latent")
    g = pipe(frames, generator=_gen(), frame_batch=8, **kw)
    assert get_unet_attn_processors(pipe.unet) == before
    e = pipe(frames, generator=_gen(), use_graph=False, **kw)
    assert get_unet_attn_processors(pipe.unet) == before
    assert g.shape == e.shape == (5, 4, 16, 16)
    r = rel_rms(g, e)
    print(f"[video graph vs eager] {start} keyframes={keyframes} strength={strength}: rel-RMS {r:.3e}")
    assert r <= GRAPH_BOUND
    assert rel_rms(g[1:2], g[0:1]) > 1e-3            # (the frames differ: the comparison is not between copies of one frame)


def test_single_keyframe_is_the_plain_cross_frame_sampler_bit_for_bit():
    """keyframes = (0,): every LOAD row is (0, 0) with alpha 0, which afldm_attention_bank runs as the single-source attention -
    the existing non-bank sampler's LOAD (afldm_attention against the one stored sample, Bk = 1) on the same stored pass."""
    from afldm_amd.harness import CrossFrameSampler
    from afldm_amd.pipelines.cross_frame_attn import set_unet_attn_processor
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = _pipeline(torch.float32)
    steps = 3
    sched = ffhq_ddim_scheduler().schedule(steps)
    lat = torch.randn(4, 4, 16, 16, generator=_gen(9)).cuda()
    out = {}
    for bank in (True, False):
        smp = CrossFrameSampler(pipe.unet, sched, steps, bank=bank)
        previous = smp.install()
        try:
            smp.run(lat[0:1], load=False)
            out[bank] = smp.run(lat, load=True, **(dict(src=[[0, 0]] * 4, alpha=[0.0] * 4) if bank else {}))
            assert set(smp.engines) == ({("bank", False, 1, 1), ("bank", True, 4, 1)} if bank else {(False, 1), (True, 4)})
        finally:
            set_unet_attn_processor(pipe.unet, dict(previous))
    print(f"[video single keyframe] max |bank - plain| = {float((out[True] - out[False]).abs().max()):.3e}")
    assert torch.equal(out[True], out[False])


def test_every_frame_a_keyframe_is_the_one_frame_call():
    pipe = _pipeline(torch.float32)
    frames = _frames(3)
    kw = dict(num_inference_steps=3, output_type="latent", frame_batch=4)
    full = pipe(frames, keyframes=(0, 1, 2), **kw)
    for f in range(3):
        one = pipe(frames[f:f + 1], keyframes=(0,), **kw)
        r = rel_rms(full[f:f + 1], one)
        print(f"[video all keyframes] frame {f}: rel-RMS against the one-frame call {r:.3e}")
        assert r <= GRAPH_BOUND


def test_keyframes_do_not_depend_on_the_frames_between_them():
    pipe = _pipeline(torch.float32)
    frames = _frames(4)
    other = frames.clone()
    other[1] = _frames(1, seed=77)[0]
    kw = dict(num_inference_steps=3, keyframes=(0, 2), output_type="latent", frame_batch=4)
    a, b = pipe(frames, **kw), pipe(other, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[3], b[3])                   # past the last keyframe: attends to keyframe 2 alone
    assert not torch.equal(a[1], b[1])


def test_chunking_one_load_graph_and_padding():
    pipe = _pipeline(torch.float32)
    frames = _frames(5)
    kw = dict(num_inference_steps=3, keyframes=(0, 3), output_type="latent")
    small = pipe(frames, frame_batch=2, **kw)
    for name, smp in _samplers(pipe).items():
        assert sorted(k for k in smp.engines) == [("bank", False, 2, 2), ("bank", True, 2, 2)], (name, list(smp.engines))
    big = pipe(frames, frame_batch=8, **kw)
    for name, smp in _samplers(pipe).items():
        assert sorted(k for k in smp.engines) == [("bank", False, 2, 2), ("bank", True, 8, 2)], (name, list(smp.engines))
    assert small.shape == big.shape == (5, 4, 16, 16)          # no padding row reaches the output
    r = rel_rms(small, big)
    print(f"[video chunking] frame_batch 2 vs 8: rel-RMS {r:.3e}")
    assert r <= GRAPH_BOUND


def test_replay_refresh_stale_model_and_evaluation_counts():
    from afldm_amd.pipelines.video_editing_pipeline import video_timesteps
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = _pipeline(torch.float32)
    frames = _frames(4)
    kw = dict(num_inference_steps=4, strength=0.8, keyframes=(0, 2), output_type="latent", frame_batch=4)
    first = pipe(frames, **kw)
    graphs = {(w, k): e.graph for w, s in _samplers(pipe).items() for k, e in s.engines.items()}
    assert len(graphs) == 4 and all(g is not None for g in graphs.values())          # two samplers x (STORE, LOAD)
    again = pipe(frames, **kw)
    assert {(w, k): e.graph for w, s in _samplers(pipe).items() for k, e in s.engines.items()} == graphs
    assert torch.equal(first, again)
    moved = pipe(_frames(4, seed=23), **kw)                     # new frames through the same graphs: the STORE pass refreshes the bank
    assert {(w, k): e.graph for w, s in _samplers(pipe).items() for k, e in s.engines.items()} == graphs
    assert rel_rms(moved, first) > 1e-2
    assert rel_rms(moved, pipe(_frames(4, seed=23), use_graph=False, **{k: v for k, v in kw.items() if k != "frame_batch"})) <= GRAPH_BOUND
    # a changed model drops the engines
    w = pipe.unet.conv_out.weight
    saved = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(1.25)
        changed = pipe(frames, **kw)
        now = {(w_, k): e.graph for w_, s in _samplers(pipe).items() for k, e in s.engines.items()}
        assert set(now) == set(graphs) and all(now[k] is not graphs[k] for k in graphs)
        assert rel_rms(changed, first) > 1e-3
    finally:
        with torch.no_grad():
            w.copy_(saved)
    assert rel_rms(pipe(frames, **kw), first) <= 1e-6
    # the eager loop evaluates the UNet as often as get_timesteps implies
    n = len(video_timesteps(ffhq_ddim_scheduler(), 4, 0.8))
    assert n == 3
    F_, S = 4, 2
    for sdedit, want in ((False, n * (1 + (F_ - S)) + n * (1 + F_)), (True, n * (1 + F_))):
        with _count_unet_calls(pipe.unet) as calls:
            pipe(frames, use_graph=False, use_sdedit=sdedit, generator=_gen(), **{k: v for k, v in kw.items() if k != "frame_batch"})
        assert len(calls) == want, (sdedit, len(calls), want)
        assert sorted(set(calls)) == [1, S] and calls.count(S) == (n if sdedit else 2 * n)


def test_bf16_unet_and_output_types():
    pipe = _pipeline(torch.bfloat16)
    frames = _frames(3)
    kw = dict(num_inference_steps=3, keyframes=(0, 2), frame_batch=2)
    lat = pipe(frames, output_type="latent", **kw)
    assert lat.shape == (3, 4, 16, 16) and lat.dtype == torch.bfloat16 and torch.isfinite(lat).all()
    pt = pipe(frames, output_type="pt", **kw)
    assert pt.shape == (3, 3, 128, 128) and torch.isfinite(pt).all()
    pil = pipe(frames, output_type="pil", **kw).images
    assert len(pil) == 3 and all(im.size == (128, 128) for im in pil)
    again = pipe(pil, output_type="latent", **kw)              # PIL frames at the model's size are accepted
    assert again.shape == (3, 4, 16, 16) and torch.isfinite(again).all()
    images, = pipe(frames, output_type="np", return_dict=False, **kw)
    assert images.shape == (3, 128, 128, 3)
    e = pipe(frames, output_type="latent", use_graph=False, **{k: v for k, v in kw.items() if k != "frame_batch"})
    print(f"[video bf16] graph vs eager rel-RMS {rel_rms(lat.float(), e.float()):.3e} (printed, not asserted)")


def test_refusals():
    from afldm_amd.pipelines.video_editing_pipeline import LDMVideoPipeline
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    pipe = _pipeline(torch.float32)
    frames = _frames(3)
    dpm = LDMVideoPipeline(pipe.vae, pipe.unet, DPMSolverMultistepScheduler.from_config(pipe.scheduler.config))
    with pytest.raises(NotImplementedError, match="DDIMScheduler"):
        dpm(frames, num_inference_steps=3)
    for bad in ((1, 2), (0, 2, 1), (0, 0), (0, 3), ()):
        with pytest.raises(ValueError, match="keyframe"):
            pipe(frames, num_inference_steps=3, keyframes=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="frame_batch"):
            pipe(frames, num_inference_steps=3, frame_batch=bad)
    with pytest.raises(ValueError, match="model's size"):
        pipe(_frames(3, size=64), num_inference_steps=3)
    with pytest.raises(ValueError, match="strength"):
        pipe(frames, num_inference_steps=3, strength=0.1)          # int(3 * 0.1) = 0 steps
    with pytest.raises(TypeError):
        pipe([], num_inference_steps=3)
    bare = LDMVideoPipeline(None, pipe.unet, pipe.scheduler)
    with pytest.raises(NotImplementedError, match="VAE"):
        bare(frames, num_inference_steps=3)
    lat = torch.randn(3, 4, 16, 16, generator=_gen(2))
    with pytest.raises(NotImplementedError, match="VAE"):
        bare(lat, num_inference_steps=3, output_type="pt")
    out = bare(lat, num_inference_steps=3, keyframes=(0, 2), output_type="latent", frame_batch=4)
    assert out.shape == (3, 4, 16, 16) and torch.isfinite(out).all()
    want = pipe(lat, num_inference_steps=3, keyframes=(0, 2), output_type="latent", frame_batch=4)
    assert torch.equal(out, want)                    # latent frames never touch the VAE
