"""The bit-reversible sampler end to end on MI355X: MyLDMPipeline.sample_reversible / invert_reversible and ReversibleEngine on the
tiny UNet (N = 6, batch 2), fp32 and bf16, replayed graphs and the eager loop.  Everything about the round trips is torch.equal
on int64; graph against eager is the one comparison with a bound (rel-RMS 1e-5, the repaint and sdedit pipeline tests' bound for
the same comparison on the same model).  One test repeats the round trip at the production shape, where the property rests on
every production kernel being run-to-run deterministic."""
import contextlib

import numpy as np
import pytest
import torch

import rev_oracle as ro
from test_gpu_dpm import build, rel_rms
from test_gpu_sde import _ldm

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
N, B = 6, 2
SHAPE = (B, 4, 16, 16)


@pytest.fixture(scope="module")
def pipes():
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = _ldm(build("tiny", dtype)[0])
        return made[dtype]
    return get


@pytest.fixture(scope="module")
def start():
    g = torch.Generator().manual_seed(5)
    return torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g) * 0.7          # noise, image latents


def encode(x):
    from afldm_amd import ops
    bad = torch.zeros(x.shape[0], dtype=torch.int32, device="cuda")
    X = ops.rev_encode(x.to("cuda", torch.float32).contiguous(), bad)
    assert not bad.any()
    return X


@contextlib.contextmanager
def taps():
    """Every ops.rev_step_flat call of the eager loop: (row, eps, far before, near before, far after, near after, lat)."""
    from afldm_amd import ops
    plain, seen = ops.rev_step_flat, []

    def tapped(far, near, eps, bad, row, out=None):
        before = (far.clone(), near.clone())
        lat = plain(far, near, eps, bad, row, out=out)
        seen.append((tuple(row), eps.clone(), *before, far.clone(), near.clone(), lat.clone()))
        return lat
    ops.rev_step_flat = tapped
    try:
        yield seen
    finally:
        ops.rev_step_flat = plain


def one_step_state(pipe, noise, use_graph):
    """X_N-1 as the sampler itself makes it from the noise: the state after its first evaluation."""
    from afldm_amd.engine import ReversibleEngine
    if not use_graph:
        with taps() as seen:
            pipe.sample_reversible_latents(latents=noise, num_inference_steps=N, use_graph=False)
        return seen[0][5]
    eng = ReversibleEngine(pipe.unet, pipe.scheduler.reversible_schedule(N, "sample", False), B, N, True)
    eng.reset(noise)
    eng.step(1)
    torch.cuda.synchronize()
    return eng.near.clone()


def test_the_same_evaluation_replayed_twice_gives_equal_bits(pipes, start):
    """The precondition of everything below."""
    from afldm_amd.engine import ReversibleEngine
    for dtype in DTYPES:
        pipe = pipes(dtype)
        eng = ReversibleEngine(pipe.unet, pipe.scheduler.reversible_schedule(N, "sample", False), B, N, True)
        a, b = eng.run(start[0]), eng.run(start[0])
        assert torch.equal(a.hi, b.hi) and torch.equal(a.lo, b.lo) and a.k == 1 and a.lo.dtype == torch.int64
        eng.reset(start[0])
        eng.step(1)
        e1 = eng.near.clone()
        eng.reset(start[0])
        eng.step(1)
        assert torch.equal(e1, eng.near)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trips_are_exact(pipes, start, dtype, use_graph):
    pipe = pipes(dtype)
    noise, image = start
    kw = dict(num_inference_steps=N, use_graph=use_graph)
    # noise -> sample -> invert: the noise's integers, and the sampler's own X_N-1 beside them
    lat, code = pipe.sample_reversible(latents=noise, output_type="latent", return_code=True, **kw)
    assert code.k == 1 and code.batch == B and code.dtype == dtype and code.num_inference_steps == N and code.strength is None
    assert lat.dtype == dtype and torch.equal(lat, code.latents().to(dtype)) and torch.isfinite(lat).all()
    back = pipe.invert_reversible(code=code, **kw)
    assert back.k == N and torch.equal(back.hi, encode(noise))
    assert torch.equal(back.lo, one_step_state(pipe, noise, use_graph))
    # image latents -> invert -> sample: the input's integers
    up = pipe.invert_reversible(image, **kw)
    assert up.k == N and not torch.equal(up.hi, encode(image))
    x0, down = pipe.sample_reversible_latents(code=up, return_code=True, **kw)
    assert down.k == 1 and torch.equal(down.lo, encode(image)) and x0.dtype == torch.float32
    assert torch.equal(x0, down.latents()) and float((x0.cpu() - image).abs().max()) <= 2.0 ** -24 * 4   # (the grid is finer than fp32 here)
    # the same part of the way: strength 0.5 is 3 evaluations up and 2 down
    half = pipe.invert_reversible(image, strength=0.5, **kw)
    assert half.k == 3 and half.strength == 0.5 and not torch.equal(half.hi, up.hi)
    _, down = pipe.sample_reversible_latents(code=half, return_code=True, **kw)
    assert torch.equal(down.lo, encode(image)) and down.strength == 0.5


@pytest.mark.parametrize("dtype", DTYPES)
def test_eager_trajectory_is_the_oracle_on_the_recorded_eps(pipes, start, dtype):
    pipe = pipes(dtype)
    with taps() as seen:
        _, code = pipe.sample_reversible_latents(latents=start[0], num_inference_steps=N, use_graph=False, return_code=True)
    assert len(seen) == N
    sched = pipe.scheduler.reversible_schedule(N, "sample", False)
    near = encode(start[0]).cpu().numpy()
    for k, (row, eps, f0, n0, f1, n1, lat) in enumerate(seen):
        assert row == sched.rows[k] and np.array_equal(n0.cpu().numpy(), near)
        wf, wn, wl, bad = ro.step(f0.cpu().numpy(), n0.cpu().numpy(), eps.cpu().numpy(), ro.f32_rows(sched)[k])
        assert not bad.any() and np.array_equal(f1.cpu().numpy(), wf) and np.array_equal(n1.cpu().numpy(), wn), k
        assert np.array_equal(lat.cpu().numpy(), wl), k
        near = wn
    assert np.array_equal(code.lo.cpu().numpy(), near) and np.array_equal(code.hi.cpu().numpy(), seen[-1][4].cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_against_eager(pipes, start, dtype):
    pipe = pipes(dtype)
    a = pipe.sample_reversible_latents(latents=start[0], num_inference_steps=N)
    b = pipe.sample_reversible_latents(latents=start[0], num_inference_steps=N, use_graph=False)
    err = rel_rms(a, b)
    print(f"[tiny reversible sampler, {N} steps, {dtype}] graph vs eager loop rel-RMS {err:.2e}, equal: {torch.equal(a, b)}")
    assert err <= 1e-5, err


def test_evaluation_counts(pipes, start):
    pipe = pipes(torch.float32)
    calls = []
    hook = pipe.unet.register_forward_hook(lambda *a: calls.append(1))
    try:
        _, code = pipe.sample_reversible_latents(latents=start[0], num_inference_steps=N, use_graph=False, return_code=True)
        assert len(calls) == N
        del calls[:]
        up = pipe.invert_reversible(code=code, num_inference_steps=N, use_graph=False)
        assert len(calls) == N - 1
        del calls[:]
        pipe.sample_reversible_latents(code=up, num_inference_steps=N, use_graph=False)
        assert len(calls) == N - 1
        del calls[:]
        pipe.invert_reversible(start[1], num_inference_steps=N, strength=0.5, use_graph=False)
        assert len(calls) == 3
    finally:
        hook.remove()
    from afldm_amd.engine import ReversibleEngine
    sch = pipe.scheduler
    assert ReversibleEngine(pipe.unet, sch.reversible_schedule(N, "sample", True), B, N - 1).n == N - 1
    with pytest.raises(ValueError):
        ReversibleEngine(pipe.unet, sch.reversible_schedule(N, "sample", True), B, N)
    with pytest.raises(NotImplementedError):
        ReversibleEngine(pipe.unet, sch.schedule(N), B, N)                  # a "ddim" schedule is not this engine's
    from afldm_amd.engine import DenoiseEngine
    with pytest.raises(NotImplementedError):
        DenoiseEngine(pipe.unet, sch.reversible_schedule(N, "sample", False), B, N)


def test_engine_cache(start):
    pipe = _ldm(build("tiny", torch.float32)[0])
    noise = start[0]
    a, code = pipe.sample_reversible_latents(latents=noise, num_inference_steps=N, return_code=True)
    (eng,) = pipe._rev_sample_start_engines.values()
    assert type(eng).__name__ == "ReversibleEngine" and eng.graph is not None
    b = pipe.sample_reversible_latents(latents=noise, num_inference_steps=N)
    assert list(pipe._rev_sample_start_engines.values())[0] is eng and torch.equal(a, b)
    # the other direction lives in a slot of its own
    pipe.invert_reversible(code=code, num_inference_steps=N)
    assert list(pipe._rev_sample_start_engines.values())[0] is eng and len(pipe._rev_invert_code_engines) == 1
    # another step count: another engine, and the first count's result is what it was
    c = pipe.sample_reversible_latents(latents=noise, num_inference_steps=N - 2)
    (other,) = pipe._rev_sample_start_engines.values()
    assert other is not eng and other.n == N - 2 and not torch.equal(a, c)
    assert torch.equal(a, pipe.sample_reversible_latents(latents=noise, num_inference_steps=N))
    # a changed model: the graphs are dropped, the result moves, and the old code is no longer this model's
    (eng,) = pipe._rev_sample_start_engines.values()
    graph = eng.graph
    with torch.no_grad():
        pipe.unet.conv_out.weight.mul_(1.5)
    d = pipe.sample_reversible_latents(latents=noise, num_inference_steps=N)
    assert list(pipe._rev_sample_start_engines.values())[0] is eng and eng.graph is not graph and not torch.equal(a, d)
    with pytest.raises(ValueError, match="model_key"):
        pipe.invert_reversible(code=code, num_inference_steps=N)
    fresh = _ldm(pipe.unet).sample_reversible_latents(latents=noise, num_inference_steps=N)
    assert torch.equal(d, fresh)


def test_steps_per_graph_1_and_2_are_bit_identical(pipes, start):
    from afldm_amd.engine import ReversibleEngine
    pipe = pipes(torch.bfloat16)
    sched = pipe.scheduler.reversible_schedule(N, "invert", False)
    got = [ReversibleEngine(pipe.unet, sched, B, N, True, steps_per_graph=k).run(start[1]) for k in (1, 2, 5)]
    for other in got[1:]:
        assert torch.equal(got[0].hi, other.hi) and torch.equal(got[0].lo, other.lo)
    assert got[0].k == N


def test_a_code_of_another_batch_size_is_refused_unless_inexact(pipes, start):
    pipe = pipes(torch.float32)
    up = pipe.invert_reversible(start[1], num_inference_steps=N)
    with pytest.raises(ValueError, match="batch"):
        pipe.sample_reversible_latents(code=up[:1], num_inference_steps=N)
    with pytest.raises(ValueError, match="level 6"):                     # another step count: the code is not at its last level
        pipe.sample_reversible_latents(code=up, num_inference_steps=N + 1)
    x0, down = pipe.sample_reversible_latents(code=up[:1], num_inference_steps=N, exact=False, return_code=True)
    assert tuple(x0.shape) == (1,) + SHAPE[1:] and down.batch == 1 and torch.isfinite(x0).all()
    print(f"[batch-2 code sampled at batch 1] differing integers: {int((down.lo != encode(start[1][:1])).sum())} of {down.lo.numel()}")


@pytest.mark.parametrize("use_graph", [True, False])
def test_a_poisoned_sample_raises_naming_its_row_only(pipes, start, use_graph):
    pipe = pipes(torch.float32)
    clean = pipe.sample_reversible_latents(latents=start[0], num_inference_steps=N, use_graph=use_graph)
    bad = start[0].clone()
    bad[1, 2, 3, 4] = float("nan")
    with pytest.raises(FloatingPointError, match=r"rows \[1\]"):
        pipe.sample_reversible_latents(latents=bad, num_inference_steps=N, use_graph=use_graph)
    assert torch.equal(clean, pipe.sample_reversible_latents(latents=start[0], num_inference_steps=N, use_graph=use_graph))


def test_every_output_type(start):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from test_gpu_vae import build_vae
    vae, _, _ = build_vae(torch.float32)
    pipe = MyLDMPipeline(vae, build("tiny", torch.float32)[0], ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    S = 16 * pipe._vae_ratio()
    kw = dict(latents=start[0], num_inference_steps=N)
    lat = pipe.sample_reversible(output_type="latent", **kw)
    pt, code = pipe.sample_reversible(output_type="pt", return_code=True, **kw)
    assert tuple(lat.shape) == SHAPE and torch.equal(lat, code.latents()) and tuple(pt.shape) == (B, 3, S, S) and torch.isfinite(pt).all()
    (arr,) = pipe.sample_reversible(output_type="np", return_dict=False, **kw)
    assert arr.shape == (B, S, S, 3) and arr.min() >= 0.0 and arr.max() <= 1.0
    out = pipe.sample_reversible(**kw)
    assert len(out.images) == B and out.images[0].size == (S, S)
    # an image goes in through the VAE's posterior mode; the draw for latents=None is __call__'s
    image = torch.nn.functional.interpolate(torch.rand(B, 3, 8, 8, generator=torch.Generator().manual_seed(2)) * 2 - 1, size=(S, S),
                                            mode="bicubic", align_corners=False).clamp(-1, 1)
    up = pipe.invert_reversible(image, num_inference_steps=N)
    _, down = pipe.sample_reversible_latents(code=up, num_inference_steps=N, return_code=True)
    assert torch.equal(down.lo, encode(pipe._encode_mode(image)))
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    drawn = pipe.sample_reversible(batch_size=B, num_inference_steps=N, generator=g1, output_type="latent")
    z = torch.randn(SHAPE, generator=g2)
    assert torch.equal(drawn, pipe.sample_reversible(latents=z, num_inference_steps=N, output_type="latent"))
    assert torch.equal(g1.get_state(), g2.get_state())


# ------------------------------------------------------------------------------------------------ the production shape
@pytest.fixture(scope="module")
def ffhq_pipe():
    from afldm_amd.af_modules.af_api import make_af_unet
    from afldm_amd.configs import FFHQ_UNET_CONFIG
    from afldm_amd.models.unet_2d import UNet2DModel
    torch.manual_seed(0)
    unet = UNet2DModel.from_config(FFHQ_UNET_CONFIG)
    with torch.no_grad():
        unet.conv_out.weight.mul_(0.1)
        unet.conv_out.bias.mul_(0.1)
    make_af_unet(unet)
    return _ldm(unet.to("cuda").to(torch.bfloat16))


def test_ffhq_bf16_batch8_round_trip_is_exact(ffhq_pipe):
    """FFHQ-size UNet, random weights, bf16, batch 8, 4 steps, replayed graphs: invert a code, sample back, every integer equal.
    Were this to fail where the tiny model passes, some production kernel is not run-to-run deterministic at this shape."""
    from afldm_amd import _lib
    from afldm_amd.engine import model_state_key
    from afldm_amd.reversible import ReversibleCode
    pipe = ffhq_pipe
    c, s = pipe.unet.config.in_channels, pipe.unet.config.sample_size
    g = torch.Generator().manual_seed(17)
    x0 = torch.randn(8, c, s, s, generator=g) * 0.7
    x1 = x0 + 0.05 * torch.randn(8, c, s, s, generator=g)
    code = ReversibleCode(encode(x1), encode(x0), 1, 4, None, 8, torch.bfloat16, model_state_key(pipe.unet), _lib.library_hash())
    up = pipe.invert_reversible(code=code, num_inference_steps=4)
    assert up.k == 4 and not torch.equal(up.hi, code.hi)
    _, down = pipe.sample_reversible_latents(code=up, num_inference_steps=4, return_code=True)
    diff_hi, diff_lo = int((down.hi != code.hi).sum()), int((down.lo != code.lo).sum())
    print(f"[FFHQ bf16 batch 8, 4 steps] differing integers after invert -> sample: hi {diff_hi}, lo {diff_lo} of {code.hi.numel()}")
    assert torch.equal(down.hi, code.hi) and torch.equal(down.lo, code.lo)
