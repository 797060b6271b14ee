"""Parallel-in-time sampling end to end on MI355X: PicardEngine and MyLDMPipeline.sample_parallel_latents on the tiny UNet with the
FFHQ DDIM scheduler against the float64 restatement of tests/picard_oracle.py on the oracle UNet, the sequential CPU sampler of
tests/slot_oracle.py, the pipeline's own sequential call, the eager launches and the torch loop.  Bounds: the project's sampler
bounds - rel-RMS <= 1e-3 for the fp32 model, <= 5e-2 for the bf16 model.

The inputs with tolerance > 0 are tests/test_picard_host.py's FIXTURE and UNEVEN: chosen on the CPU so that no error of a run is
near its threshold, and asserted there.

Measured on MI355X (rel-RMS):
  test 1, fp32, tolerance 0, windows 1 / 3 / 4, 1 and 2 images: 1.19e-7 ... 1.25e-7 against the CPU sampler; against
          pipe(batch_size=1): 0 (bit-identical) at UNet batches 1, 2, 3 and 4, 7.7e-8 at batches 6 and 8 (the UNet's own rounding at another batch size)
  test 2, the fixture, strides [[1, 1], [1, 1], [3, 3], [1, 1]] as the oracle's: 1.25e-7 on the graphs, 1.24e-7 in the torch loop
  test 4, tolerance 0, window 3: fp32 1.25e-7, after unet.to(torch.bfloat16) 3.2e-4
  test 5, 4-step inversion, window 3, against pipe.ddim_inversion: 3.5e-7"""
import pytest
import torch

import picard_oracle as po
import slot_oracle as so
from test_gpu_sde import _ldm
from test_gpu_unet import build, rel_rms
from test_picard_host import FIXTURE, UNEVEN, start

pytestmark = pytest.mark.gpu

N = 6


@pytest.fixture(scope="module")
def tiny32():
    return build("tiny", torch.float32)


def _schedule(n):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    return ffhq_ddim_scheduler().schedule(n)


@pytest.fixture(scope="module")
def sequential(tiny32):
    """The CPU sampler's float64 latents of the two fixture seeds, 6 steps: computed once, shared, never written."""
    _, cfg, sd = tiny32
    return torch.cat([so.sample(sd, cfg, start((s,)), _schedule(N)) for s in FIXTURE["seeds"]])


def _engine(unet, n, P, window, tolerance, use_graph=True, steps_per_graph=5):
    from afldm_amd.engine import PicardEngine
    return PicardEngine(unet, _schedule(n), P, n, use_graph, steps_per_graph, window=window, tolerance=tolerance)


# ------------------------------------------------------------------------------------------------ 1. tolerance 0
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("window", [1, 3, 4])
def test_tolerance_zero_is_the_sequential_sampler(tiny32, sequential, window, P):
    pipe = _ldm(tiny32[0])
    x = start(FIXTURE["seeds"][:P])
    got, stats = pipe.sample_parallel_latents(num_inference_steps=N, window=window, tolerance=0.0, latents=x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (P, 4, 16, 16) and got.is_cuda
    assert stats["iterations"] == N and stats["evaluations"] == N * P * window and stats["strides"] == [[1] * P] * N
    e_oracle = rel_rms(got, sequential[:P])
    one = torch.cat([pipe(batch_size=1, num_inference_steps=N, latents=x[p:p + 1], output_type="latent") for p in range(P)])
    e_pipe = rel_rms(got, one.float().cpu())
    print(f"[picard] fp32, tolerance 0, window {window}, {P} image(s): rel-RMS against the CPU sampler {e_oracle:.2e}, against "
          f"pipe(batch_size=1) {e_pipe:.2e} (bit-identical: {torch.equal(got, one.float())})")
    assert e_oracle <= 1e-3 and e_pipe <= 1e-3
    eng, = pipe._picard_engines.values()
    assert eng.graph is not None and eng.graph_multi is not None and eng.branches == 1
    eager = _engine(tiny32[0], N, P, window, 0.0, use_graph=False).run(x)
    assert torch.equal(got, eager), "graph replay must be bit-identical to eager launches"
    for spg in (1, 2):
        assert torch.equal(got, _engine(tiny32[0], N, P, window, 0.0, steps_per_graph=spg).run(x)), spg


# ------------------------------------------------------------------------------------------------ 2. tolerance > 0
def test_fixture_strides_and_latents_against_the_oracle(tiny32):
    unet, cfg, sd = tiny32
    f = FIXTURE
    pipe = _ldm(unet)
    x, sched = start(f["seeds"]), _schedule(f["steps"])
    want, strides, _ = po.sample(po.unet_eps(sd, cfg, sched), x, sched, f["window"], f["tolerance"])
    for use_graph in (True, False):
        got, stats = pipe.sample_parallel_latents(num_inference_steps=f["steps"], window=f["window"], tolerance=f["tolerance"],
                                                  latents=x, use_graph=use_graph)
        err = rel_rms(got, want)
        print(f"[picard] fixture, use_graph={use_graph}: strides {stats['strides']}, rel-RMS against the oracle {err:.2e}")
        assert stats["strides"] == strides and stats["iterations"] == len(strides)
        assert stats["evaluations"] == len(strides) * 2 * f["window"]
        assert got.dtype == torch.float32 and err <= 1e-3


# ------------------------------------------------------------------------------------------------ 3. a finished image is left alone
def test_two_images_finish_after_different_counts(tiny32):
    f = UNEVEN
    x = start(f["seeds"])
    eng = _engine(tiny32[0], f["steps"], 2, f["window"], f["tolerance"], steps_per_graph=1)
    eng.reset(x)
    eng.step(2)
    base, done = eng._poll()
    assert done == 2 and base[0] == f["steps"] and base[1] < f["steps"], (base, done)
    first = eng.states[:, 0].clone()
    rows, t_cur = eng.temb_rows[0::2].clone(), eng.t_cur[0::2].clone()
    eng.step(2)                                                         # one more than the second image needs
    base, done = eng._poll()
    assert done == 4 and base == [f["steps"]] * 2
    assert torch.equal(eng.states[:, 0], first) and torch.equal(eng.temb_rows[0::2], rows) and torch.equal(eng.t_cur[0::2], t_cur)
    got = eng.run(x)
    assert eng.stats["strides"] == [[1, 1], [3, 2], [0, 1]] and eng.stats["iterations"] == 3
    assert torch.equal(got[0], first[0])
    print(f"[picard] two images, strides {eng.stats['strides']}: the first one's states keep their bits through the extra iterations")


# ------------------------------------------------------------------------------------------------ 4. the bf16 model
def test_bf16_model(sequential):
    unet, _, _ = build("tiny", torch.float32)
    x = start(FIXTURE["seeds"])
    eng = _engine(unet, N, 2, 3, 0.0)
    got = eng.run(x)
    graph = eng.graph
    unet.to(torch.bfloat16)
    got16 = eng.run(x)                                                  # the same engine: re-allocated in the new dtype, re-captured
    assert eng.x_nhwc.dtype == eng.temb_rows.dtype == torch.bfloat16 and eng.graph is not None and eng.graph is not graph
    e32, e16 = rel_rms(got, sequential), rel_rms(got16, sequential)
    print(f"[picard] tolerance 0, window 3: rel-RMS against the CPU sampler fp32 {e32:.2e}, after unet.to(torch.bfloat16) {e16:.2e}")
    assert e32 <= 1e-3 and e16 <= 5e-2 and eng.stats["iterations"] == N and got16.dtype == torch.float32
    got_p, stats = _ldm(unet).sample_parallel_latents(num_inference_steps=N, window=3, tolerance=0.0, latents=x)
    assert torch.equal(got_p, got16) and stats["iterations"] == N


# ------------------------------------------------------------------------------------------------ 5. inversion
def test_inversion_schedule(tiny32):
    from afldm_amd.engine import PicardEngine
    pipe = _ldm(tiny32[0])
    pipe.scheduler.set_timesteps(4)
    inv = pipe.inversion_schedule()
    x = start((50, 51))
    want = pipe.ddim_inversion(x.cuda(), bar=False)
    eng = PicardEngine(tiny32[0], inv, 2, 4, window=3, tolerance=0.0)
    got = eng.run(x)
    err = rel_rms(got, want.cpu())
    print(f"[picard] 4-step inversion, window 3, tolerance 0: rel-RMS against pipe.ddim_inversion {err:.2e}")
    assert err <= 1e-3 and eng.stats["iterations"] == 4


# ------------------------------------------------------------------------------------------------ what the engine refuses
def test_refusals(tiny32):
    from afldm_amd.engine import PicardEngine
    from afldm_amd.pipelines.cross_frame_attn import (AttnState, CrossFrameAttnProcessor, get_unet_attn_processors,
                                                      set_unet_attn_processor)
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    with pytest.raises(NotImplementedError, match="'sde'"):
        PicardEngine(tiny32[0], ffhq_ddim_scheduler().stochastic_schedule(3, 0.5), 1, 3)
    with pytest.raises(ValueError, match="window"):
        _engine(tiny32[0], 4, 1, 0, 0.0)
    eng = _engine(tiny32[0], 4, 1, 2, 0.0)
    with pytest.raises(ValueError, match="latents"):
        eng.run(torch.zeros(2, 4, 16, 16))
    unet, _, _ = build("tiny", torch.float32)
    state = AttnState()
    set_unet_attn_processor(unet, {k: CrossFrameAttnProcessor(state) for k in get_unet_attn_processors(unet)})
    with pytest.raises(ValueError, match="plain one"):
        _engine(unet, 4, 1, 2, 0.0)


# ------------------------------------------------------------------------------------------------ 6. the surface
def test_sample_parallel_and_the_engine_cache(tiny32):
    pipe = _ldm(tiny32[0])
    g = lambda: torch.Generator().manual_seed(40)          # noqa: E731
    out = pipe.sample_parallel(batch_size=2, num_inference_steps=4, window=2, tolerance=0.0, generator=g(), output_type="latent")
    assert tuple(out.shape) == (2, 4, 16, 16) and out.dtype == tiny32[0].dtype and out.is_cuda
    assert pipe.parallel_stats["iterations"] == 4
    # the start latents are __call__'s
    want = pipe(batch_size=2, num_inference_steps=4, generator=g(), output_type="latent")
    assert rel_rms(out, want.cpu()) <= 1e-3
    eng, = pipe._picard_engines.values()
    graph = eng.graph
    again = pipe.sample_parallel(batch_size=2, num_inference_steps=4, window=2, tolerance=0.0, generator=g(), output_type="latent")
    now, = pipe._picard_engines.values()
    assert now is eng and eng.graph is graph and torch.equal(again, out)
    with pytest.raises(NotImplementedError, match="VAE"):
        pipe.sample_parallel(num_inference_steps=2, window=2)
