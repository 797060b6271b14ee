"""Stochastic samplers on the graph-replayed engine (MI355X): afldm_sde_step against torch, stochastic DDIM and the stochastic /
clipped I2SB bridge on replayed graphs against their own eager loops (same generator, same draws) on the tiny UNet, and
against the oracle UNet driven by the oracle schedulers at FFHQ size.  fp32: 1e-3 against the oracle (the DDIM trajectory
tests' bound); bf16: 1.5x the error the deterministic graph path reaches against the oracle on the same inputs."""
import itertools
import math

import pytest
import torch

from test_gpu_dpm import build, rel_rms

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
INF = math.inf
ROWS = [
    (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.0, 0.7, 0.5, 0.3),        # DDIM-shaped: no clip, direction and noise
    (1.0, -0.9, -1.0, 1.0, 0.4, 0.55, 0.0, 0.2),                 # I2SB-shaped: clipped, no direction term
    (1.0, 0.0, -0.5, 0.5, 0.0, 1.0, 0.0, 0.0),                   # x_out = clamp(x, -0.5, 0.5), exactly
]


def torch_sde(x, e, z, row):
    p, q, lo, hi, a, b, d, c = row
    return a * x + b * torch.clamp(p * x + q * e, lo, hi) + d * e + c * z


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("dtype,hw", list(itertools.product(DTYPES, [16, 5])))    # 16-byte groups / the scalar form
def test_sde_step_kernel(dtype, hw):
    from afldm_amd import ops
    B, C = 3, 4
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, C, hw, hw, generator=g)
    x[0, 0, 0, :4] = torch.tensor([0.5, -0.5, 0.75, -3.0])            # on and beyond the bounds of row 2
    x[1, 2, 1, 3] = math.nan                                          # NaN passes through every row, as torch.clamp passes it
    e = torch.randn(B, C, hw, hw, generator=g).to(dtype).float()       # what the kernel reads
    e_nhwc = e.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)
    # the noise rows as a batch slice of a larger buffer (a branch of the engine): row stride 2 B C H W
    big = torch.randn(len(ROWS), 2 * B, C, hw, hw, generator=g)
    noise = big.cuda()[:, B:]
    coef = torch.tensor(ROWS, dtype=torch.float32).reshape(-1).cuda()
    for s, row in enumerate(ROWS):
        idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
        xg = x.cuda()
        out = ops.sde_step(xg, e_nhwc, noise, coef, idx, advance=False, out=xg)     # x_out aliases x
        assert out.data_ptr() == xg.data_ptr() and int(idx.item()) == s
        want = torch_sde(x, e, big[s, B:], [float(v) for v in torch.tensor(row, dtype=torch.float32)])
        got = out.cpu()
        assert torch.isnan(got[1, 2, 1, 3]) and torch.isnan(got).sum() == 1, s
        torch.testing.assert_close(got, want, rtol=2e-6, atol=2e-6 * float(want.nan_to_num().abs().max()), equal_nan=True)
        if s == 2:
            assert got[0, 0, 0, :4].tolist() == [0.5, -0.5, 0.5, -0.5]
    # advance: the kernel reads row 0, then the counter moves on; a second launch reads row 1
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    ops.sde_step(xg, e_nhwc, noise, coef, idx, advance=True, out=xg)
    ops.sde_step(xg, e_nhwc, noise, coef, idx, advance=True, out=xg)
    assert int(idx.item()) == 2
    want = torch_sde(torch_sde(x, e, big[0, B:], ROWS[0]), e, big[1, B:], ROWS[1])
    torch.testing.assert_close(xg.cpu(), want, rtol=1e-5, atol=1e-5 * float(want.nan_to_num().abs().max()), equal_nan=True)


# ------------------------------------------------------------------------------------------------ tiny UNet
def _ldm(unet):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _i2sb(unet, clip=True):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    from afldm_amd.schedulers.i2sb import I2SBScheduler
    cfg = {k: v for k, v in FFHQ_DDIM_CONFIG.items() if k != "set_alpha_to_one"}
    pipe = I2SBLDMPipeline(None, unet, I2SBScheduler.from_config(dict(cfg, clip_sample=clip)))
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _gens(kind, seed):
    if kind == "cpu":
        return torch.Generator().manual_seed(seed)
    if kind == "cuda":
        return torch.Generator("cuda").manual_seed(seed)
    return [torch.Generator().manual_seed(seed + i) for i in range(2)]


def _state(g):
    return [x.get_state() for x in g] if isinstance(g, list) else [g.get_state()]


def _same_state(a, b):
    return all(torch.equal(u, v) for u, v in zip(_state(a), _state(b)))


@pytest.mark.parametrize("kind", ["cpu", "cuda", "list"])
def test_tiny_ddim_eta_graph_vs_eager_loop(kind):
    unet, _, _ = build("tiny", torch.float32)
    pipe = _ldm(unet)
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    ga, gb, gc = _gens(kind, 11), _gens(kind, 11), _gens(kind, 11)
    a = pipe(latents=x, eta=0.7, num_inference_steps=8, generator=ga, output_type="latent")
    (key,) = pipe._engines
    assert key[5] == "DDIMScheduler" and pipe._engines[key].schedule.kind == "sde"
    b = pipe(latents=x, eta=0.7, num_inference_steps=8, generator=gb, output_type="latent", use_graph=False)
    err = rel_rms(a, b.float())
    print(f"[tiny DDIM eta=0.7, 8 steps, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe(latents=x, eta=0.7, num_inference_steps=8, generator=gc, output_type="latent"))
    det = pipe(latents=x, num_inference_steps=8, output_type="latent")
    assert rel_rms(det, a) > 1e-2                                      # the noise did enter


@pytest.mark.parametrize("kind", ["cpu", "cuda", "list"])
def test_tiny_i2sb_stochastic_clipped_graph_vs_eager_loop(kind):
    unet, _, _ = build("tiny", torch.float32)
    pipe = _i2sb(unet, clip=True)
    start = (0.8 * torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(5))).cuda()
    ga, gb, gc = _gens(kind, 99), _gens(kind, 99), _gens(kind, 99)
    a = pipe._bridge(start, 10, False, ga)
    assert "_ode_engines" not in pipe.__dict__ and len(pipe._sde_engines) == 1
    b = pipe._bridge(start, 10, False, gb, use_graph=False)
    err = rel_rms(a, b)
    print(f"[tiny I2SB stochastic clipped, 9 evaluations, {kind} generator] graph vs eager loop rel-RMS {err:.2e}")
    assert err <= 1e-5, err
    assert _same_state(ga, gb)
    assert torch.equal(a, pipe._bridge(start, 10, False, gc))
    # the clipped ODE draws nothing
    g = _gens(kind, 1)
    before = _state(g)
    c = pipe._bridge(start, 10, True, g)
    assert all(torch.equal(u, v) for u, v in zip(before, _state(g)))
    assert rel_rms(c, pipe._bridge(start, 10, True, None, use_graph=False)) <= 1e-5


@pytest.mark.parametrize("which", ["ddim", "i2sb"])
def test_tiny_sde_engine_eager_replay_and_branches(which, monkeypatch):
    from afldm_amd import trunk
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, _, _ = build("tiny", torch.float32)
    if which == "ddim":
        sde = ffhq_ddim_scheduler().stochastic_schedule(8, 0.7)
    else:
        sde = _i2sb(unet).scheduler.bridge_schedule(10, False)
    n = len(sde.rows)
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4))

    def run(use_graph):
        eng = DenoiseEngine(unet, sde, 2, n, use_graph=use_graph)
        assert eng.noise is not None and tuple(eng.noise.shape) == (n, 2, 4, 16, 16)
        g = torch.Generator().manual_seed(8)
        return eng.run(x, draw=sde.drawer(g, (2, 4, 16, 16), torch.device("cuda"), unet.dtype))
    graph = run(True)
    assert torch.equal(run(False), graph), "graph replay must be bit-identical to the engine's eager launches"
    with pytest.raises(ValueError):
        DenoiseEngine(unet, sde, 2, n, use_graph=True).run(x)          # no draw: an error, not zero noise
    monkeypatch.setattr(trunk, "_BLOCKED", set(trunk._BLOCKED))
    monkeypatch.setenv("AFLDM_BRANCHES", "2")
    eng2 = DenoiseEngine(unet, sde, 2, n, use_graph=True)
    assert eng2.branches == 2
    two = eng2.run(x, draw=sde.drawer(torch.Generator().manual_seed(8), (2, 4, 16, 16), torch.device("cuda"), unet.dtype))
    print(f"[tiny {which} sde engine] AFLDM_BRANCHES=2 vs 1: bit-equal {torch.equal(two, graph)}, rel-RMS {rel_rms(two, graph):.2e}")
    assert torch.equal(two, graph)


# ------------------------------------------------------------------------------------------------ FFHQ-size UNet vs the oracle
def _oracle_ddim(sd, cfg, x, steps, eta, seed, draw_dtype=torch.float32):
    """The oracle UNet driven by oracle.ddim.DDIM.  The oracle draws its noise in eps's dtype (fp32); diffusers' step - and the
    product - draw in the model output's dtype, so a bf16 model's noise is drawn in bf16 (other values, same generator
    consumption): draw_dtype replays that draw inside the oracle's step and widens it to fp32."""
    from oracle import ddim as od, unet as ou
    o = od.DDIM()
    o.set_timesteps(steps)
    gen = torch.Generator().manual_seed(seed)
    real = torch.randn

    def randn(*a, dtype=None, **k):
        return real(*a, dtype=draw_dtype, **k).to(dtype or torch.float32)
    lat = x.clone()
    torch.randn = randn
    try:
        for t in o.timesteps:
            lat = o.step(ou.unet_forward(sd, cfg, lat, t), t, lat, eta=eta, generator=gen)
    finally:
        torch.randn = real
    return lat


def _oracle_i2sb(sd, cfg, start, steps, is_ode, clip, seed):
    from oracle import i2sb as oi, unet as ou
    o = oi.I2SB(clip_sample=clip)
    o.set_timesteps(steps)
    gen = torch.Generator().manual_seed(seed)
    lat = start.clone()
    for t in o.timesteps[:steps - 1]:
        lat = o.step(ou.unet_forward(sd, cfg, lat, t), t, lat, is_ode=is_ode, generator=gen)
    return lat


@pytest.fixture(scope="module")
def ffhq_setup():
    from oracle import configs as oc, unet as ou
    cfg = oc.FFHQ_UNET
    sd = ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(21))
    start = 0.8 * torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(22))
    return cfg, sd, x, start


@pytest.mark.parametrize("dtype", DTYPES)
def test_ffhq_ddim_eta1_vs_oracle(ffhq_setup, dtype):
    cfg, sd, x, _ = ffhq_setup
    unet, _, _ = build("ffhq", dtype)
    pipe = _ldm(unet)
    got = pipe(latents=x, eta=1.0, num_inference_steps=20, generator=torch.Generator().manual_seed(31), output_type="latent")
    err = rel_rms(got.float(), _oracle_ddim(sd, cfg, x, 20, 1.0, 31, draw_dtype=dtype))
    if dtype == torch.float32:
        print(f"[FFHQ DDIM eta=1, 20 steps, batch 2] fp32 rel-RMS vs oracle {err:.3e}")
        assert err <= 1e-3, err
        return
    det = rel_rms(pipe(latents=x, num_inference_steps=20, output_type="latent").float(), _oracle_ddim(sd, cfg, x, 20, 0.0, 31))
    print(f"[FFHQ DDIM 20 steps, batch 2] bf16 rel-RMS vs oracle: eta=1 {err:.3e}, eta=0 (graph path) {det:.3e}")
    assert err <= 1.5 * det, (err, det)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ffhq_i2sb_stochastic_clipped_vs_oracle(ffhq_setup, dtype):
    cfg, sd, _, start = ffhq_setup
    unet, _, _ = build("ffhq", dtype)
    got = _i2sb(unet, clip=True)._bridge(start.cuda(), 21, False, torch.Generator().manual_seed(41))
    err = rel_rms(got, _oracle_i2sb(sd, cfg, start, 21, False, True, 41))
    if dtype == torch.float32:
        print(f"[FFHQ I2SB stochastic clipped, 20 evaluations, batch 2] fp32 rel-RMS vs oracle {err:.3e}")
        assert err <= 1e-3, err
        return
    det = rel_rms(_i2sb(unet, clip=False)._bridge(start.cuda(), 21, True, None), _oracle_i2sb(sd, cfg, start, 21, True, False, 0))
    print(f"[FFHQ I2SB 20 evaluations, batch 2] bf16 rel-RMS vs oracle: stochastic clipped {err:.3e}, unclipped ODE {det:.3e}")
    assert err <= 1.5 * det, (err, det)
