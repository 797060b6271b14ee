"""Perturbed-attention guidance, host side (no GPU): the oracle (tests/pag_oracle.py) - an empty site set is the plain oracle UNet
bit for bit, the folded one-GEMM identity block equals the unfolded chain in float64, the guided update's limits - the "pag"
schedule (rows, draws, key), the layer-name matching of MyLDMPipeline.pag_sites with its two ValueErrors, the bindings, and that
the guidance separates from the unguided sample on the tiny oracle UNet at the settings the GPU tests compare at."""
import math
import os

import pytest
import torch

import pag_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = ("up_blocks.1", "up_blocks.2")


def sched(**kw):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    return DDIMScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)


def tiny():
    from oracle import configs as oc, unet as ou
    cfg = oc.tiny_unet()
    return cfg, ou.randomize_norm_affine(ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1))      # test_gpu_dpm.build("tiny")


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------------ oracle
def test_no_sites_is_the_plain_oracle_and_the_core_is_restored():
    from oracle import unet as ou
    cfg, sd = tiny()
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    core = ou._attention_core
    plain = ou.unet_forward(sd, cfg, x, 501)
    assert torch.equal(po.unet_forward_perturbed(sd, cfg, x, 501, ()), plain)
    assert ou._attention_core is core
    sites = ou.attention_sites(cfg)
    assert len(sites) == 7
    pert = po.unet_forward_perturbed(sd, cfg, x, 501, UP)
    assert ou._attention_core is core and not torch.equal(pert, plain)
    with pytest.raises(RuntimeError):
        with po.perturbed_attention(UP):
            raise RuntimeError("inside")
    assert ou._attention_core is core                                      # also after an exception
    assert torch.equal(ou.unet_forward(sd, cfg, x, 501), plain)


def test_folded_block_equals_the_unfolded_chain_in_float64():
    cfg, sd = tiny()
    from oracle import unet as ou
    g = torch.Generator().manual_seed(5)
    for prefix in ou.attention_sites(cfg):
        c = sd[prefix + ".to_v.weight"].shape[0]
        x = torch.randn(3, c, 4, 4, generator=g, dtype=torch.float64) * 2 + 0.5
        sd64 = {k: v.double() for k, v in sd.items() if k.startswith(prefix)}
        a = po.identity_block(sd64, prefix, x, cfg["norm_num_groups"], cfg["norm_eps"])
        b = po.identity_block_folded(sd, prefix, x, cfg["norm_num_groups"], cfg["norm_eps"])
        assert a.dtype == b.dtype == torch.float64
        assert float((a - b).abs().max() / a.abs().max()) <= 1e-12, prefix


def test_pag_step_limits():
    g = torch.Generator().manual_seed(7)
    x, e, ep, z = (torch.randn(3, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(4))
    base = (1 / 0.6, -0.8 / 0.6, -math.inf, math.inf, 0.1, 0.7, 0.5, 0.3)
    p, q, lo, hi, a, b, d, c = base
    sde = a * x + b * torch.clamp(p * x + q * e, lo, hi) + d * e + c * z
    assert torch.equal(po.pag_step(x, e, ep, z, base + (0.0, 0.0, 0.0, 0.0)), sde)          # s = 0, phi = 0: the sde update of e
    # phi = 1: the rescaled g has e's standard deviation, per sample (read back through a row that returns g itself)
    ident = (0.0, 0.0, -math.inf, math.inf, 0.0, 0.0, 1.0, 0.0)
    gres = po.pag_step(x, e, ep, None, ident + (3.0, 1.0, 0.0, 0.0))
    torch.testing.assert_close(gres.std(dim=(1, 2, 3)), e.std(dim=(1, 2, 3)), rtol=1e-12, atol=0)
    graw = po.pag_step(x, e, ep, None, ident + (3.0, 0.0, 0.0, 0.0))
    assert torch.equal(graw, e + 3.0 * (e - ep))
    half = po.pag_step(x, e, ep, None, ident + (3.0, 0.5, 0.0, 0.0))
    want = graw * (0.5 * e.std(dim=(1, 2, 3), keepdim=True) / graw.std(dim=(1, 2, 3), keepdim=True) + 0.5)
    torch.testing.assert_close(half, want, rtol=1e-12, atol=0)
    # sigma(g) = 0: the ratio is 1, nothing is NaN
    e0 = e.clone()
    e0[1] = 0.0
    out = po.pag_step(x, e0, e0, None, ident + (3.0, 0.7, 0.0, 0.0))
    assert torch.isfinite(out).all() and torch.equal(out[1], torch.zeros_like(out[1]))


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("n", [4, 50])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_pag_schedule_rows_draws_and_key(n, eta):
    from afldm_amd.schedulers.schedule import NOISE_SLOTS, ROW_WIDTH
    assert ROW_WIDTH["pag"] == 12 and NOISE_SLOTS["pag"] == 1
    pag = sched().pag_schedule(n, eta, 3.0, 0.7)
    sde = sched().stochastic_schedule(n, eta)
    assert pag.kind == "pag" and pag.timesteps == sde.timesteps and len(pag.rows) == n
    for r, w in zip(pag.rows, sde.rows):
        assert r[:8] == w and r[8:] == (3.0, 0.7, 0.0, 0.0)                # float for float
    assert torch.equal(pag.table("cpu")[:, :8], sde.table("cpu"))
    if eta:
        assert pag.draws == sde.draws and all(pag.draws)                    # the same draws as the stochastic sampler
        assert [pag.slots(k) for k in range(n)] == [sde.slots(k) for k in range(n)]
    else:
        assert not any(pag.draws) and all(r[7] == 0.0 for r in pag.rows)    # eta = 0: c = 0 and nothing is drawn
    other = sched().pag_schedule(n, eta, 2.0, 0.7)
    assert other.key != pag.key and other.rows[0][8] == 2.0
    assert sched().pag_schedule(n, eta, 3.0, 0.0).key != pag.key
    assert sched().pag_schedule(n, eta, 3.0, 0.7) is pag                    # the same settings: the same schedule
    assert pag.key != sde.key
    with pytest.raises(ValueError):
        sched().pag_schedule(n, eta, -1.0, 0.0)
    with pytest.raises(ValueError):
        sched().pag_schedule(n, eta, 3.0, 1.5)


def test_pag_draws_are_the_eager_steps_draws():
    pag = sched().pag_schedule(4, 0.7, 3.0, 0.0)
    sde = sched().stochastic_schedule(4, 0.7)
    ga, gb = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    da = pag.drawer(ga, (2, 4, 16, 16), torch.device("cpu"), torch.float32)
    db = sde.drawer(gb, (2, 4, 16, 16), torch.device("cpu"), torch.float32)
    for k in range(4):
        for _ in pag.slots(k):
            assert torch.equal(da(), db())
    assert torch.equal(ga.get_state(), gb.get_state())


# ------------------------------------------------------------------------------------------------ layer names
def _cpu_pipe():
    from afldm_amd.models.unet_2d import UNet2DModel
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    cfg, _ = tiny()
    pipe = MyLDMPipeline(None, UNet2DModel.from_config(cfg), ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe, cfg


def test_layer_names_match_on_dot_boundaries():
    from oracle import unet as ou
    from afldm_amd.pipelines.cross_frame_attn import get_unet_attn_processors
    pipe, cfg = _cpu_pipe()
    every = tuple(sorted(ou.attention_sites(cfg)))
    assert tuple(sorted(k[:-len(".processor")] for k in get_unet_attn_processors(pipe.unet))) == every
    assert pipe.pag_sites(("mid_block",)) == ("mid_block.attentions.0",)
    assert pipe.pag_sites("mid_block") == ("mid_block.attentions.0",)
    assert pipe.pag_sites(("up_blocks.1",)) == tuple(s for s in every if s.startswith("up_blocks.1."))
    assert pipe.pag_sites(("up_blocks.1.attentions.0",)) == ("up_blocks.1.attentions.0",)
    assert pipe.pag_sites(("up_blocks", "down_blocks", "mid_block")) == every
    assert pipe.pag_sites(()) == ()
    for bad in ("mid", "up_blocks.1.attentions.0.processor", "up_blocks.1.att", "up_blocks.9", "", "mid_block."):
        with pytest.raises(ValueError):
            pipe.pag_sites((bad,))
    before = get_unet_attn_processors(pipe.unet)
    with pytest.raises(ValueError):                                        # an unknown name, before anything runs
        pipe.pag_latents(latents=torch.zeros(1, 4, 16, 16), pag_applied_layers=("nowhere",), num_inference_steps=2)
    with pytest.raises(ValueError):                                        # an empty selection with a positive scale
        pipe.pag_latents(latents=torch.zeros(1, 4, 16, 16), pag_applied_layers=(), pag_scale=3.0, num_inference_steps=2)
    after = get_unet_attn_processors(pipe.unet)
    assert all(after[k] is before[k] for k in before)


def test_dpm_schedulers_are_refused():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    pipe, _ = _cpu_pipe()
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG)
    for call in (pipe.pag_latents, pipe.pag):
        with pytest.raises(NotImplementedError):
            call(latents=torch.zeros(1, 4, 16, 16), num_inference_steps=2)


# ------------------------------------------------------------------------------------------------ bindings
def test_pag_entry_points_are_bound_and_documented():
    from afldm_amd import _lib, build, ops
    names = ("afldm_attn_identity_block", "afldm_attn_identity_block_ok", "afldm_pag_step", "afldm_pag_step_flat")
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in names:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name + "(" in hdr and name in doc
    assert "pag.hip" in build.SOURCES
    for f in ("attn_identity_block_ok", "attn_identity_block", "pag_step", "pag_step_flat"):
        assert callable(getattr(ops, f))
    # host arithmetic of the query: bf16 (code 1), 32 groups, the listed token counts and widths
    ok = _lib.lib.afldm_attn_identity_block_ok
    for T in (4, 16, 64, 256, 1024):
        for C in (64, 128, 192, 384, 768):
            assert ok(3, T, C, 32, 1) == 1 and ok(3, T, C, 32, 0) == 0
    assert ok(1, 32, 128, 32, 1) == 0 and ok(1, 64, 256, 32, 1) == 0 and ok(1, 64, 128, 16, 1) == 0 and ok(0, 64, 128, 32, 1) == 0
    # refusals before any launch: NULL pointers, and a sample above the element limit
    lib = _lib.lib
    assert lib.afldm_pag_step(None, None, None, 0, None, None, None, 0, 1, 4, 8, 8, 0, None) == -5
    assert lib.afldm_attn_identity_block(None, None, 1, None, None, 32, 1e-5, None, None, None, 1, 4, 64, 1, None) == -5
    # no CPU path
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError):
        ops.pag_step_flat(x, x, x, None, (1.0, 0.0, -1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0))


# ------------------------------------------------------------------------------------------------ the guidance separates
def test_guidance_separates_on_the_tiny_oracle():
    """The settings the GPU tests compare at must move the sample by more than their 1e-3 bound can hide: more than 1e-2 against
    the unguided sample, and more than 1e-2 between guidance_rescale 0 and 0.7."""
    cfg, sd = tiny()
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    runs = {}
    for s, phi in ((0.0, 0.0), (3.0, 0.0), (3.0, 0.7)):
        runs[s, phi] = po.sample(sd, cfg, x, sched().pag_schedule(4, 0.0, s, phi), UP)
    from oracle import unet as ou
    plain = x.double()
    for t, row in zip(sched().pag_schedule(4, 0.0, 0.0, 0.0).timesteps, sched().stochastic_schedule(4, 0.0).rows):
        e = ou.unet_forward(sd, cfg, plain.float(), int(t))
        plain = po.pag_step(plain, e, e, None, row + (0.0, 0.0))
    assert torch.equal(runs[0.0, 0.0], plain)                              # s = 0: the unguided sampler
    d_guided, d_rescale = rel_rms(runs[3.0, 0.0], plain), rel_rms(runs[3.0, 0.7], runs[3.0, 0.0])
    print(f"[tiny oracle, 4 steps, {UP}] s = 3 vs unguided {d_guided:.2e}; phi 0.7 vs 0 {d_rescale:.2e}")
    assert d_guided > 1e-2 and d_rescale > 1e-2
