"""Two-image interpolation (reference afldm/pipelines/image_interpolation_pipeline.py:284-766, warp_method 3) on MI355X:
the blended two-source attention kernel (afldm_attention_interp) against fp64 torch, its graph replay with new blend weights,
the cached interpolating processor against the oracle fixture, LDMInterpolationPipeline end to end against its eager
statement-by-statement path and the oracle, and the packed-weight regression of ADVICE r06 item 1."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FFHQ_LEVELS = [(1024, 192, 8), (256, 384, 16), (64, 384, 16), (16, 768, 32), (4, 768, 32)]   # (T, C, heads), head_dim 24


def rel_rms(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def _operands(B, Bk, T, C, dtype, seed):
    """q, k0, k1 as column views of wider buffers (as the fused projection leaves them), vt0 / vt1 channel-major."""
    g = torch.Generator().manual_seed(seed)
    qbuf = torch.randn(B, T, 3 * C, generator=g).to(device="cuda", dtype=dtype)
    kbuf0 = torch.randn(Bk, T, 2 * C, generator=g).to(device="cuda", dtype=dtype)
    kbuf1 = torch.randn(Bk, T, 2 * C, generator=g).to(device="cuda", dtype=dtype)
    vt0 = torch.randn(Bk, C, T, generator=g).to(device="cuda", dtype=dtype)
    vt1 = torch.randn(Bk, C, T, generator=g).to(device="cuda", dtype=dtype)
    return qbuf[:, :, :C], kbuf0[:, :, C:], vt0, kbuf1[:, :, C:], vt1


def _reference(q, k0, vt0, k1, vt1, alpha, heads):
    """fp64: (1 - alpha) sdpa(q, k0, v0) + alpha sdpa(q, k1, v1), kv-sample b // (B / Bk)."""
    B, T, C = q.shape
    Bk, d = k0.shape[0], C // heads

    def sdpa(k, vt):
        kk = k.double().repeat_interleave(B // Bk, 0).view(B, -1, heads, d).transpose(1, 2)
        vv = vt.double().transpose(1, 2).repeat_interleave(B // Bk, 0).reshape(B, -1, heads, d).transpose(1, 2)
        return F.scaled_dot_product_attention(q.double().view(B, T, heads, d).transpose(1, 2), kk, vv).transpose(1, 2).reshape(B, T, C)
    a = alpha.double().view(B, 1, 1)
    return (1 - a) * sdpa(k0, vt0) + a * sdpa(k1, vt1)


def _alphas(B):
    return torch.tensor([0.37]) if B == 1 else torch.linspace(0, 1, B)       # per sample, exact 0 and 1 included


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("T,C,heads", FFHQ_LEVELS + [(256, 64, 8), (256, 128, 8), (256, 256, 8)])
def test_attention_interp_vs_torch(dtype, tol, T, C, heads):
    """Every FFHQ attention level (head_dim 24) and head_dim 8 / 16 / 32 at 16^2; B in {1, 3, 17} against one stored sample,
    and two stored samples (Bk = 2: the batch repeat); alpha = 0 / 1 is ops.attention on source 0 / 1 bit for bit."""
    from afldm_amd import ops
    for B, Bk in ((1, 1), (3, 1), (17, 1), (2, 2), (4, 2)):
        q, k0, vt0, k1, vt1 = _operands(B, Bk, T, C, dtype, seed=T + C + B)
        alpha = _alphas(B).cuda()
        o = ops.attention_interp(q, k0, vt0, k1, vt1, alpha, heads)
        assert o.shape == (B, T, C) and o.dtype == dtype
        r = rel_rms(o, _reference(q, k0, vt0, k1, vt1, alpha, heads))
        assert r <= tol, (B, Bk, r)
        # alpha = 0 / 1: the single-source launch on source 0 / 1, bit for bit ((1 - 0) / l == 1 / l, ob + 0 * o1 == ob, and
        # source 1 restarts as a fresh launch)
        zero, one = torch.zeros(B, device="cuda"), torch.ones(B, device="cuda")
        assert torch.equal(ops.attention_interp(q, k0, vt0, k1, vt1, zero, heads), ops.attention(q, k0, vt0, heads)), (B, Bk)
        assert torch.equal(ops.attention_interp(q, k0, vt0, k1, vt1, one, heads), ops.attention(q, k1, vt1, heads)), (B, Bk)


def test_attention_interp_rejects_bad_operands():
    from afldm_amd import ops
    q, k0, vt0, k1, vt1 = _operands(2, 1, 64, 192, torch.float32, seed=1)
    with pytest.raises(ValueError, match="alpha"):
        ops.attention_interp(q, k0, vt0, k1, vt1, torch.zeros(3, device="cuda"), 8)
    with pytest.raises(ValueError, match="differ"):
        ops.attention_interp(q, k0, vt0, k1.contiguous(), vt1, torch.zeros(2, device="cuda"), 8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_interp_graph_replay_reads_new_alpha(dtype):
    """The blend weights are read when the kernel runs: a captured launch replayed after the alpha buffer changed gives the
    eager result for the new weights, bit for bit."""
    from afldm_amd import ops
    B, T, C, heads = 5, 256, 384, 16
    q, k0, vt0, k1, vt1 = _operands(B, 1, T, C, dtype, seed=3)
    alpha = torch.zeros(B, device="cuda")
    out = torch.empty(B, T, C, device="cuda", dtype=dtype)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.attention_interp(q, k0, vt0, k1, vt1, alpha, heads, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.attention_interp(q, k0, vt0, k1, vt1, alpha, heads, out=out)
    for vals in ([0.0, 0.25, 0.5, 0.75, 1.0], [1.0, 0.9, 0.1, 0.0, 0.6]):
        alpha.copy_(torch.tensor(vals))
        g.replay()
        want = ops.attention_interp(q, k0, vt0, k1, vt1, torch.tensor(vals, device="cuda"), heads)
        torch.cuda.synchronize()
        assert torch.equal(out, want), vals


# ----------------------------------------------------------------------------------------------- processor on the fixture
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2)])
def test_cached_interp_processor_vs_oracle_fixture(golden, dtype, tol, monkeypatch):
    """test_enable_interp_vs_oracle through the NEW path: one batch-2 two-slot STORE of interp_xa | interp_xb, then a cached
    LOAD of interp_xc with per-sample alpha (one afldm_attention_interp launch per attention); mixed alpha equals scalar runs."""
    from test_gpu_r02 import build_unet
    from afldm_amd import ops
    from afldm_amd.pipelines.cross_frame_attn import (AttnState, CrossFrameAttnProcessor, get_unet_attn_processors,
                                                      set_unet_attn_processor)
    g = golden("g11_r02.npz")
    unet, _, _ = build_unet("tiny", dtype)
    state = AttnState()
    procs = {k: CrossFrameAttnProcessor(state, enable_interp=True, cache_kv=True) for k in get_unet_attn_processors(unet)}
    set_unet_attn_processor(unet, dict(procs))
    calls = []
    real = ops.attention_interp
    monkeypatch.setattr(ops, "attention_interp", lambda *a, **k: calls.append(1) or real(*a, **k))
    state.reset()
    state.set_timestep(501)
    state.set_store_id(AttnState.PAIR)
    unet(torch.cat([torch.from_numpy(g["interp_xa"]), torch.from_numpy(g["interp_xb"])]).cuda(), 501)
    for p in procs.values():
        assert p.kv[0][501][0].shape[0] == 1 and p.kv[1][501][0].shape[0] == 1
    state.to_load()
    xc = torch.from_numpy(g["interp_xc"]).cuda()
    state.set_alpha(torch.full((2,), 0.3, device="cuda"))
    assert rel_rms(unet(xc, 501, return_dict=False)[0], g["interp_y"]) <= tol
    assert len(calls) == len(procs)
    state.set_alpha(torch.zeros(2, device="cuda"))
    assert rel_rms(unet(xc, 501, return_dict=False)[0], g["interp_y_alpha0"]) <= tol
    x3 = torch.cat([xc, xc[:1].flip(-1)])
    state.set_alpha(torch.tensor([0.0, 0.3, 1.0], device="cuda"))
    mixed = unet(x3, 501, return_dict=False)[0]
    for i, a in enumerate((0.0, 0.3, 1.0)):
        state.set_alpha(a)
        one = unet(x3[i:i + 1], 501, return_dict=False)[0]
        assert rel_rms(mixed[i:i + 1], one) <= tol, i


# ----------------------------------------------------------------------------------------------- pipeline end to end
def _tiny_pipeline(dtype, unet_name="tiny", vae_dtype=None):
    from test_gpu_r02 import build_unet
    from test_gpu_vae import build_vae
    from afldm_amd.pipelines.image_interpolation_pipeline import LDMInterpolationPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, ucfg, usd = build_unet(unet_name, dtype)
    vae, vcfg, vsd = build_vae(vae_dtype or dtype)
    pipe = LDMInterpolationPipeline(vae, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe, (ucfg, usd, vcfg, vsd)


def _images(size, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [F.interpolate(torch.rand(1, 3, 8, 8, generator=g) * 2 - 1, size=(size, size), mode="bicubic",
                          align_corners=False).clamp(-1, 1) for _ in range(2)]


@torch.no_grad()
def _oracle_frames(ucfg, usd, vcfg, vsd, images, n, steps):
    """The reference procedure on the oracle: posterior mean, DDIM inversion per image, restated slerp, two batch-1 STORE
    passes, a per-frame batch-1 LOAD with scalar alpha f / (n - 1) (AttnCache(enable_interp=True))."""
    from oracle import pipeline as op, unet as ou, vae as ov
    from oracle.ddim import DDIM
    inv = []
    for x in images:
        z = ov.encode_moments(vsd, vcfg, x)[:, :4] * vcfg["scaling_factor"]
        inv.append(op.ddim_inversion(usd, ucfg, z, steps))
    fr = torch.linspace(0, 1, n)
    lat = torch.empty((n,) + tuple(inv[0].shape[1:]))
    lat[0], lat[-1] = inv[0][0], inv[1][0]
    for i in range(1, n - 1):
        p0, p1 = lat[0].double(), lat[-1].double()
        dot = (torch.sum(p0 * p1) / (torch.linalg.norm(p0) * torch.linalg.norm(p1))).clamp(-1 + 1e-7, 1 - 1e-7)
        th = torch.arccos(dot)
        lat[i] = (p0 * torch.sin(th - th * fr[i]) / torch.sin(th) + p1 * torch.sin(th * fr[i]) / torch.sin(th)).float()
    return _oracle_passes(ucfg, usd, lat, steps)


@torch.no_grad()
def _oracle_passes(ucfg, usd, lat, steps):
    """Steps 5-6 of the reference procedure on the oracle, from the frames' initial latents lat [n, C, H, W] (CPU fp32)."""
    from oracle import unet as ou
    from oracle.ddim import DDIM
    n = lat.shape[0]
    cache = ou.AttnCache(enable_interp=True)
    cache.state = ou.AttnCache.STORE
    for sid, z in ((0, lat[0:1]), (1, lat[-1:])):
        cache.store_id = sid
        s = DDIM()
        s.set_timesteps(steps)
        for t in s.timesteps:
            cache.timestep = int(t)
            z = s.step(ou.unet_forward(usd, ucfg, z, t, cache=cache), t, z, eta=0.0)
    cache.state = ou.AttnCache.LOAD
    s = DDIM()
    s.set_timesteps(steps)
    for t in s.timesteps:
        cache.timestep = int(t)
        eps = []
        for f in range(n):
            cache.alpha = f / (n - 1)
            eps.append(ou.unet_forward(usd, ucfg, lat[f:f + 1], t, cache=cache))
        lat = s.step(torch.cat(eps), t, lat, eta=0.0)
    return lat


@contextlib.contextmanager
def _count_interp_launches():
    """Records the batch of every ops.attention_interp call made inside the block."""
    from afldm_amd import ops
    calls, real = [], ops.attention_interp

    def counted(q, *a, **k):
        calls.append(q.shape[0])
        return real(q, *a, **k)
    ops.attention_interp = counted
    try:
        yield calls
    finally:
        ops.attention_interp = real


# (graph vs oracle, eager vs oracle, graph vs eager); measured fp32 9.1e-8 / 9.3e-8 / 8.2e-8, bf16 3.1e-4 / 5.2e-3 / 5.2e-3 (the
# eager loop stores the latents in bf16 between steps, the graph path in fp32)
@pytest.mark.parametrize("dtype,tols", [(torch.float32, (1e-6, 1e-6, 1e-6)), (torch.bfloat16, (3e-3, 2e-2, 2e-2))])
def test_interpolation_passes_vs_eager_and_oracle(dtype, tols):
    """Steps 5-6 alone (two-slot STORE graph, per-sample-alpha LOAD graph) from the same initial frames, tiny UNet, 5 frames,
    10 steps: against the reference loop (use_graph=False's passes, latents in the UNet's dtype) and the oracle.  Without the
    inversion in front, bf16 is held to the fixed bounds: the graph path against the eager loop and against the oracle."""
    from afldm_amd.pipelines.image_interpolation_pipeline import interp_alphas
    n, steps = 5, 10
    pipe, (ucfg, usd, _, _) = _tiny_pipeline(dtype, vae_dtype=torch.float32)
    ends = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(21))
    fracs, weights = interp_alphas(n)
    lat = pipe._frames(ends[0:1].cuda(), ends[1:2].cuda(), n, fracs, True)
    with _count_interp_launches() as calls:
        g = pipe._graph_passes(ends.cuda(), lat, steps, weights)
    (smp,) = pipe._xframe_interp_sampler.values()
    assert len(calls) == (steps + 1) * len(smp.procs)
    e = pipe._eager_passes(lat.to(dtype), steps, weights)
    want = _oracle_passes(ucfg, usd, lat.cpu(), steps)
    r_ge, r_go, r_eo = rel_rms(g, e.float()), rel_rms(g, want), rel_rms(e.float(), want)
    print(f"[interp passes, {dtype}, {steps} steps] graph vs eager {r_ge:.2e}, graph vs oracle {r_go:.2e}, eager vs oracle {r_eo:.2e}")
    assert all(r <= t for r, t in zip((r_go, r_eo, r_ge), tols)), ((r_go, r_eo, r_ge), tols)


@pytest.mark.parametrize("steps", [6, 50])
def test_interpolation_pipeline_vs_eager_and_oracle(steps):
    """Tiny UNet + tiny AF-VAE, 5 frames: the graph path, use_graph=False and the oracle; frame 0 / n-1 are plain DDIM samples
    of the inverted endpoints (alpha 0 / 1 attends to the frame's own stored pass)."""
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.pipelines.cross_frame_attn import get_unet_attn_processors
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    n = 5
    images = _images(128)
    pipe, (ucfg, usd, vcfg, vsd) = _tiny_pipeline(torch.float32)
    before = get_unet_attn_processors(pipe.unet)
    tm = {}
    with _count_interp_launches() as calls:
        g = pipe(*images, num_frames=n, num_inference_steps=steps, output_type="latent", timings=tm)
    # the LOAD graph's capture (a warm-up step + every step) runs every attention site through afldm_attention_interp
    assert len(calls) == (steps + 1) * len(before) and set(calls) == {n}
    assert g.shape == (n, 4, 16, 16) and tm["unet_s"] > 0 and tm["vae_s"] > 0
    assert get_unet_attn_processors(pipe.unet) == before
    e = pipe(*images, num_frames=n, num_inference_steps=steps, output_type="latent", use_graph=False)
    assert get_unet_attn_processors(pipe.unet) == before
    r_ge = rel_rms(g, e)
    want = _oracle_frames(ucfg, usd, vcfg, vsd, images, n, steps)
    r_go, r_eo = rel_rms(g, want), rel_rms(e, want)
    print(f"[interp tiny, {steps} steps] graph vs eager {r_ge:.2e}, graph vs oracle {r_go:.2e}, eager vs oracle {r_eo:.2e}")
    assert r_ge <= 1e-4 and r_go <= 1e-3 and r_eo <= 1e-3
    # endpoints = plain sampling of the inverted latents (no processors)
    lat = pipe.image2latent(torch.cat(images)).float()
    pipe.scheduler.set_timesteps(steps)
    inv = pipe.ddim_inversion(lat, bar=False)
    plain = DenoiseEngine(pipe.unet, ffhq_ddim_scheduler(), 2, steps).run(inv)
    assert rel_rms(g[0:1], plain[0:1]) <= 1e-4 and rel_rms(g[-1:], plain[1:2]) <= 1e-4
    # bf16 UNet (the VAE's bf16 error is pinned by test_gpu_vae): the same call against the fp32 oracle
    pipe16, _ = _tiny_pipeline(torch.bfloat16, vae_dtype=torch.float32)
    b = pipe16(*images, num_frames=n, num_inference_steps=steps, output_type="latent")
    b_e = pipe16(*images, num_frames=n, num_inference_steps=steps, output_type="latent", use_graph=False)
    r16, r16e, r16ge = rel_rms(b.float(), want), rel_rms(b_e.float(), want), rel_rms(b.float(), b_e.float())
    print(f"[interp tiny, {steps} steps] bf16 UNet: graph vs oracle {r16:.2e}, eager (the reference procedure in bf16) vs oracle "
          f"{r16e:.2e}, graph vs eager {r16ge:.2e}")
    # inversion + resampling doubles the bf16 chain of test_ddim_inversion_vs_oracle (5e-2 for the inversion alone): the whole
    # call is held to the reference procedure's own bf16 error (+25 %); test_interpolation_passes_vs_eager_and_oracle holds the
    # graph-specific part (STORE / LOAD graphs, the kernel) in bf16 to fixed bounds without the inversion in front
    assert r16 <= 1.25 * r16e + 5e-3


def test_interpolation_pipeline_ffhq_size_vs_oracle():
    """FFHQ-size AF-UNet (fp32) + tiny AF-VAE: 3 frames over a 4-step schedule against the oracle."""
    n, steps = 3, 4
    images = _images(256, seed=5)
    pipe, (ucfg, usd, vcfg, vsd) = _tiny_pipeline(torch.float32, unet_name="ffhq")
    with _count_interp_launches() as calls:
        got = pipe(*images, num_frames=n, num_inference_steps=steps, output_type="latent")
    (smp,) = pipe._xframe_interp_sampler.values()
    assert len(calls) == (steps + 1) * len(smp.procs)
    r = rel_rms(got, _oracle_frames(ucfg, usd, vcfg, vsd, images, n, steps))
    print(f"[interp FFHQ size, 3 frames, 4 steps] graph vs oracle {r:.2e}")
    assert r <= 1e-3


def test_interpolation_pipeline_outputs_and_rejections():
    pipe, _ = _tiny_pipeline(torch.float32)
    images = _images(128, seed=3)
    imgs = pipe(*images, num_frames=3, num_inference_steps=3, output_type="pil").images
    assert len(imgs) == 3 and imgs[0].size == (128, 128)
    pt = pipe(*images, num_frames=3, num_inference_steps=3, output_type="pt")
    assert pt.shape == (3, 3, 128, 128) and torch.isfinite(pt).all()
    with pytest.raises(NotImplementedError, match="GMFlow"):
        pipe(*images, num_frames=3, warp_method=0)
    with pytest.raises(ValueError, match="num_frames"):
        pipe(*images, num_frames=1)


# ----------------------------------------------------------------------------------------------- ADVICE r06 item 1
def test_sampler_first_run_keeps_the_inversion_graphs_weights():
    """Capture a ddim_inversion graph, then run a new sampler's first STORE: the packed-weight tensors the inversion graph
    points at must still be the UNet's packed weights (the first run used to count as a model change and free them).  The
    same after an in-place weight change that both notice.  Consecutive pipeline calls (inversion graph -> sampler ->
    inversion graph replay) give bit-equal frames, before and after a weight change."""
    from afldm_amd.harness import CrossFrameSampler
    from afldm_amd.pipelines.cross_frame_attn import set_unet_attn_processor
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe, _ = _tiny_pipeline(torch.float32)
    unet = pipe.unet
    pipe.scheduler.set_timesteps(3)
    lat = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(2)).cuda()
    pipe.ddim_inversion(lat, bar=False)
    packed = [(m, k, v) for m in unet.modules() for k, v in m.__dict__.get("_afldm_cache", {}).items()]
    assert packed
    smp = CrossFrameSampler(unet, ffhq_ddim_scheduler(), 3, interp=True)
    prev = smp.install()
    try:
        smp.run(lat, load=False)
    finally:
        set_unet_attn_processor(unet, dict(prev))
    for m, k, v in packed:
        assert m.__dict__.get("_afldm_cache", {}).get(k) is v, (type(m).__name__, k)
    # a real weight change: the inversion engine notices first, repacks and re-captures; the sampler, noticing next, must not
    # drop the copies that graph now points at
    with torch.no_grad():
        unet.conv_in.weight.mul_(1.25)
    pipe.ddim_inversion(lat, bar=False)
    packed = [(m, k, v) for m in unet.modules() for k, v in m.__dict__.get("_afldm_cache", {}).items()]
    prev = smp.install()
    try:
        smp.run(lat, load=False)
    finally:
        set_unet_attn_processor(unet, dict(prev))
    for m, k, v in packed:
        assert m.__dict__.get("_afldm_cache", {}).get(k) is v, ("after a weight change", type(m).__name__, k)
    images = _images(128, seed=9)
    a = pipe(*images, num_frames=4, num_inference_steps=3, output_type="latent")
    b = pipe(*images, num_frames=4, num_inference_steps=3, output_type="latent")
    assert torch.equal(a, b)
    (smp,) = pipe._xframe_interp_sampler.values()
    assert sorted(smp.engines) == [("interp", False, 2), ("interp", True, 4)]
    with torch.no_grad():
        unet.conv_in.weight.mul_(0.8)
    c = pipe(*images, num_frames=4, num_inference_steps=3, output_type="latent")
    d = pipe(*images, num_frames=4, num_inference_steps=3, output_type="latent")
    assert not torch.equal(a, c) and torch.equal(c, d)
