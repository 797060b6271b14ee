"""Self-attention guidance, host side (no GPU): the blur taps against a restatement of diffusers' gaussian_blur_2d, the oracle's
pieces (tests/sag_oracle.py) against torch - reflect padding, nearest up-sampling, the two algebraic forms of the degraded input in
float64, the mass identities - the "sag" schedule, the draws, the refusals, the site resolution, that sag_scale = 0 is the plain
DDIM oracle trajectory, that the guidance separates from it by more than the GPU tests' 1e-3 bound could hide, and THE MARGIN
CONDITION: the mask is a threshold, so every closed-loop configuration the GPU tests compare at must keep every oracle mass at
least 1e-4 away from 1."""
import os

import pytest
import torch
import torch.nn.functional as F

import pag_oracle as po
import sag_oracle as so
from test_pag_host import _cpu_pipe, rel_rms, sched, tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ taps and the oracle's pieces
@pytest.mark.parametrize("n,sigma", [(9, 1.0), (1, 1.0), (15, 1.0), (5, 0.7), (15, 3.0)])
def test_taps_are_diffusers_window_rounded_once(n, sigma):
    from afldm_amd import ops
    taps = ops.gaussian_taps(n, sigma)
    # diffusers gaussian_blur_2d, restated: linspace(-k, k, steps) / sigma -> exp(-x^2 / 2) -> normalised
    half = (n - 1) * 0.5
    x = torch.linspace(-half, half, steps=n, dtype=torch.float64)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    want = (pdf / pdf.sum()).float()
    assert len(taps) == n and torch.equal(torch.tensor(taps, dtype=torch.float64), want.double())      # fp32 values, exactly
    assert abs(sum(taps) - 1.0) <= n * 2.0 ** -24 and taps == taps[::-1]
    assert torch.equal(so.gaussian_window(n, sigma).float(), want)
    for bad in ((8, 1.0), (17, 1.0), (0, 1.0), (9, 0.0)):
        with pytest.raises(ValueError):
            ops.gaussian_taps(*bad)


@pytest.mark.parametrize("boundary", ["reflect", "circular"])
def test_blur_boundaries_against_pad(boundary):
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 8, 8, generator=g, dtype=torch.float64)
    w = so.gaussian_window(9, 1.0)
    got = so.gaussian_blur_2d(img, w, boundary)
    # separable restatement with explicit index arithmetic: reflect without edge repeat, or wrap
    H = img.shape[-1]
    idx = torch.arange(-4, H + 4)
    idx = idx % H if boundary == "circular" else torch.where(idx < 0, -idx, torch.where(idx >= H, 2 * (H - 1) - idx, idx))
    assert torch.equal(F.pad(img, [4] * 4, mode=boundary), img[..., idx, :][..., :, idx])
    rows = sum(w[t] * img[..., :, idx[t:t + H]] for t in range(9))
    want = sum(w[t] * rows[..., idx[t:t + H], :] for t in range(9))
    assert float((got - want).abs().max()) <= 1e-14
    if boundary == "circular":                                             # the degradation commutes with circular shifts
        assert float((so.gaussian_blur_2d(img.roll((3, -2), (-2, -1)), w, boundary) - got.roll((3, -2), (-2, -1))).abs().max()) <= 1e-14
    one = torch.ones(1, dtype=torch.float64)
    assert torch.equal(so.gaussian_blur_2d(img, one, boundary), img)      # one tap: the identity


def test_mask_upsampling_is_nearest_by_the_integer_ratio():
    g = torch.Generator().manual_seed(2)
    for hm, H in ((2, 8), (4, 16), (8, 32), (16, 16), (64, 64)):
        mask = torch.rand(3, hm * hm, generator=g) > 0.5
        up = so.upsampled_mask(mask, H, H)
        r = H // hm
        Y, X = torch.meshgrid(torch.arange(H), torch.arange(H), indexing="ij")
        want = mask[:, (Y // r) * hm + X // r].double()[:, None]           # latent (Y, X) reads token (Y // r) hm + X // r
        assert torch.equal(up, want)
        assert torch.equal(up, F.interpolate(mask.view(3, 1, hm, hm).double(), (H, H), mode="nearest"))


@pytest.mark.parametrize("boundary", ["reflect", "circular"])
def test_the_two_forms_of_the_degraded_input_agree_in_float64(boundary):
    g = torch.Generator().manual_seed(3)
    x, e = (torch.randn(2, 4, 16, 16, generator=g, dtype=torch.float64) for _ in range(2))
    mask = torch.rand(2, 16, generator=g) > 0.5
    w = so.gaussian_window()
    for row in sched().sag_schedule(4, 0.0, 0.75, 0.0).rows:
        a = so.degrade(x, e, mask, row[0], row[1], w, boundary)
        b = so.degrade_product_form(x, e, mask, row[0], row[1], w, boundary)
        assert float((a - b).abs().max()) <= 1e-13 * float(a.abs().max())
        M = so.upsampled_mask(mask, 16, 16).expand_as(x) > 0
        assert torch.equal(b[~M], x[~M]) and not torch.equal(b[M], x[M])    # unmasked elements are x itself
    nothing = torch.zeros(2, 16, dtype=torch.bool)
    assert float((so.degrade(x, e, nothing, 1.25, -0.75, w, boundary) - x).abs().max()) <= 1e-14


def test_mass_identities():
    g = torch.Generator().manual_seed(4)
    B, T, heads, d = 2, 64, 4, 8
    q, k = (torch.randn(B, T, heads * d, generator=g) for _ in range(2))
    mass = so.key_mass(q, k, heads)
    assert mass.shape == (B, T) and mass.dtype == torch.float64
    torch.testing.assert_close(mass.sum(1), torch.full((B,), float(T), dtype=torch.float64), rtol=1e-13, atol=0)
    # diffusers' spelling on the explicit map
    P = torch.softmax(q.double().view(B, T, heads, d).transpose(1, 2) @ k.double().view(B, T, heads, d).permute(0, 2, 3, 1) * d ** -0.5, -1)
    assert torch.equal(mass, P.mean(1).sum(1))
    # a uniform map (q = 0): every mass is 1 up to rounding, the strict threshold at exactly-1 masks nothing
    uniform = so.key_mass(torch.zeros_like(q), k, heads)
    assert float((uniform - 1.0).abs().max()) <= 1e-14
    ones = torch.ones(B, T, dtype=torch.float64)
    assert not (ones > 1.0).any() and not (torch.full((B, T), float("nan")) > 1.0).any()
    x, e = (torch.randn(B, 4, 16, 16, generator=g, dtype=torch.float64) for _ in range(2))
    assert torch.equal(so.degrade_product_form(x, e, ones > 1.0, 1.25, -0.75, so.gaussian_window()), x)


def test_observed_attention_leaves_the_oracle_unet_as_found():
    from oracle import unet as ou
    cfg, sd = tiny()
    x = so.start_latents(3, 2)
    core = ou._attention_core
    plain = ou.unet_forward(sd, cfg, x, 501)
    for site, T in (("mid_block.attentions.0", 16), ("up_blocks.1.attentions.0", 64), ("up_blocks.2.attentions.1", 256)):
        with so.observed_attention(site) as seen:
            assert torch.equal(ou.unet_forward(sd, cfg, x, 501), plain)      # observing changes nothing
        assert ou._attention_core is core and seen["calls"] == 1 and seen["mass"].shape == (2, T)
        torch.testing.assert_close(seen["mass"].sum(1), torch.full((2,), float(T), dtype=torch.float64), rtol=1e-12, atol=0)
    with pytest.raises(RuntimeError):
        with so.observed_attention("mid_block.attentions.0"):
            raise RuntimeError("inside")
    assert ou._attention_core is core


# ------------------------------------------------------------------------------------------------ schedule, draws, refusals
@pytest.mark.parametrize("n", [4, 50])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_sag_rows_are_pag_rows(n, eta):
    from afldm_amd.schedulers.schedule import NOISE_SLOTS, ROW_WIDTH
    assert ROW_WIDTH["sag"] == 12 and NOISE_SLOTS["sag"] == 1
    sag = sched().sag_schedule(n, eta, 0.75, 0.3)
    pag = sched().pag_schedule(n, eta, 0.75, 0.3)
    assert sag.kind == "sag" and pag.kind == "pag" and sag.key != pag.key
    assert sag.timesteps == pag.timesteps and sag.rows == pag.rows and sag.draws == pag.draws      # float for float
    assert torch.equal(sag.table("cpu"), pag.table("cpu"))
    assert sched().sag_schedule(n, eta, 0.75, 0.3) is sag and sched().sag_schedule(n, eta, 1.0, 0.3).key != sag.key
    ab = sched().alphas_cumprod
    for t, row in zip(sag.timesteps, sag.rows):                            # p = 1 / sqrt(abar_t), q = -sqrt(1 - abar_t) / sqrt(abar_t)
        a = float(ab[t])
        assert abs(row[0] - a ** -0.5) <= 1e-6 * a ** -0.5 and abs(row[1] + ((1 - a) / a) ** 0.5) <= 1e-6 * abs(row[1])
    for bad in ((-1.0, 0.0), (0.75, 1.5)):
        with pytest.raises(ValueError):
            sched().sag_schedule(n, eta, *bad)


def test_sag_draws_are_pag_draws():
    sag = sched().sag_schedule(4, 0.7, 0.75, 0.0)
    pag = sched().pag_schedule(4, 0.7, 0.75, 0.0)
    ga, gb = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    da = sag.drawer(ga, (2, 4, 16, 16), torch.device("cpu"), torch.float32)
    db = pag.drawer(gb, (2, 4, 16, 16), torch.device("cpu"), torch.float32)
    for k in range(4):
        assert sag.slots(k) == pag.slots(k) == (0,)
        assert torch.equal(da(), db())
    assert torch.equal(ga.get_state(), gb.get_state())
    assert not any(sched().sag_schedule(4, 0.0, 0.75, 0.0).draws)


def test_site_resolution_and_refusals():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.pipelines.cross_frame_attn import get_unet_attn_processors
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    pipe, cfg = _cpu_pipe()
    assert pipe.sag_site_of("mid_block") == "mid_block.attentions.0"
    assert pipe.sag_site_of("mid_block.attentions.0") == "mid_block.attentions.0"
    assert pipe.sag_site_of("up_blocks.1.attentions.0") == "up_blocks.1.attentions.0"
    for bad in ("up_blocks.1", "up_blocks", "mid", "nowhere", "", "mid_block.", "up_blocks.1.attentions.0.processor",
                ("mid_block",), None):
        with pytest.raises(ValueError) as err:
            pipe.sag_site_of(bad)
        assert "mid_block.attentions.0" in str(err.value) and "up_blocks.1.attentions.0" in str(err.value)      # the candidates
    before = get_unet_attn_processors(pipe.unet)
    x = torch.zeros(1, 4, 16, 16)
    for kw in (dict(sag_site="up_blocks.1"), dict(blur_kernel_size=8), dict(blur_kernel_size=17), dict(blur_sigma=0.0),
               dict(blur_boundary="zeros"), dict(masks=[torch.zeros(1, 16, dtype=torch.bool)] * 2),      # masks with use_graph=True
               dict(return_masks=True), dict(sag_scale=-1.0), dict(guidance_rescale=2.0),
               dict(masks=[torch.zeros(1, 16, dtype=torch.bool)], use_graph=False),                        # one mask for two steps
               dict(latents=torch.zeros(1, 4, 8, 8))):
        with pytest.raises(ValueError):
            pipe.sag_latents(**dict(dict(latents=x, num_inference_steps=2), **kw))
    after = get_unet_attn_processors(pipe.unet)
    assert all(after[k] is before[k] for k in before)
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG)
    for call in (pipe.sag_latents, pipe.sag):
        with pytest.raises(NotImplementedError):
            call(latents=x, num_inference_steps=2)


def test_sag_entry_points_are_bound_and_documented():
    from afldm_amd import _lib, build, ops
    names = ("afldm_attn_key_mass", "afldm_attn_key_mass_ok", "afldm_sag_degrade", "afldm_sag_degrade_flat")
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in names:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name + "(" in hdr and name in doc
    assert "sag.hip" in build.SOURCES
    for f in ("attn_key_mass_ok", "attn_key_mass", "sag_degrade", "sag_degrade_flat", "gaussian_taps"):
        assert callable(getattr(ops, f))
    ok = _lib.lib.afldm_attn_key_mass_ok
    for T in (4, 16, 64, 256, 1024):
        for d in (8, 16, 24, 32):
            assert ok(3, 32, T, d, _lib.BF16) == 1 and ok(3, 1, T, d, _lib.F32) == 1
    assert ok(1, 8, 12, 16, _lib.BF16) == 0 and ok(1, 8, 64, 40, _lib.BF16) == 0 and ok(0, 8, 64, 16, _lib.BF16) == 0
    assert ok(1, 0, 64, 16, _lib.BF16) == 0 and ok(1, 8, 64, 16, 7) == 0
    lib = _lib.lib
    assert lib.afldm_attn_key_mass(None, 64, None, 64, None, None, 1, 4, 16, 16, 0.25, _lib.F32, None) == -5      # NULL pointers
    assert lib.afldm_sag_degrade(None, None, None, None, None, None, None, 9, 0, 1, 4, 16, 16, 4, _lib.F32, None) == -5
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError):                                      # no CPU path
        ops.sag_degrade_flat(x, x, torch.zeros(1, 4), ops.gaussian_taps(), "reflect", 1.0, 0.0)
    with pytest.raises(RuntimeError):
        ops.attn_key_mass(torch.zeros(1, 16, 32), torch.zeros(1, 16, 32), 2)


# ------------------------------------------------------------------------------------------------ the oracle loop
def test_scale_zero_is_the_plain_ddim_oracle_trajectory():
    from oracle import unet as ou
    cfg, sd = tiny()
    x = so.start_latents(2, 2)
    got, masses = so.sample(sd, cfg, x, sched().sag_schedule(4, 0.0, 0.0, 0.0), "up_blocks.1.attentions.0")
    plain = x.double()
    for t, row in zip(sched().schedule(4).timesteps, sched().stochastic_schedule(4, 0.0).rows):
        e = ou.unet_forward(sd, cfg, plain.float(), int(t))
        plain = po.pag_step(plain, e, e, None, row + (0.0, 0.0))
    assert torch.equal(got, plain) and len(masses) == 4
    # ... which is DDIMScheduler.step's trajectory (x0 form) in float64
    ddim, ab = x.double(), sched().alphas_cumprod.double()
    ts = list(sched().schedule(4).timesteps)
    for i, t in enumerate(ts):
        e = ou.unet_forward(sd, cfg, ddim.float(), int(t)).double()
        a_t, a_p = ab[t], (ab[ts[i + 1]] if i + 1 < len(ts) else sched().final_alpha_cumprod.double())
        x0 = (ddim - (1 - a_t).sqrt() * e) / a_t.sqrt()
        ddim = a_p.sqrt() * x0 + (1 - a_p).sqrt() * e
    assert rel_rms(got, ddim) <= 1e-6


@pytest.mark.parametrize("name", sorted(so.CLOSED_LOOPS))
def test_margin_condition_and_separation_of_the_closed_loops(name):
    """Every closed-loop fp32 configuration of tests/test_gpu_sag_pipeline.py: the float64 oracle loop's own min |mass - 1| over all
    evaluations, samples and keys is at least 1e-4 (a configuration that misses is replaced by another seed, never excused), and
    the guided sample differs from the plain one by at least 1e-2 rel-RMS, so that the 1e-3 bound can see the feature."""
    cfg, sd = tiny()
    site, seed, steps, B, scale, eta, gseed = so.CLOSED_LOOPS[name]
    x, z, masses, margin = so.closed_loop(name, sd, cfg)
    plain, _ = so.sample(sd, cfg, x, sched().sag_schedule(steps, eta, 0.0, 0.0), site)
    moved = rel_rms(z, plain)
    masked = sum(int((m > 1.0).sum()) for m in masses) / sum(m.numel() for m in masses)
    print(f"[tiny oracle SAG {name}: {site}, seed {seed}, {steps} steps, B {B}, scale {scale}] margin {margin:.3e}; guidance moves the "
          f"sample by {moved:.3e}; {100 * masked:.0f} % of the keys masked")
    assert len(masses) == steps and margin >= so.MARGIN, margin
    assert moved >= 1e-2, moved
    assert 0.0 < masked < 1.0


@pytest.mark.parametrize("kind", ["cpu", "list"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_margin_condition_of_the_graph_against_eager_configurations(eta, kind):
    cfg, sd = tiny()
    _, masses, margin = so.graph_loop(sd, cfg, eta, kind)
    print(f"[tiny oracle SAG graph-vs-eager configuration eta={eta} {kind} generator] margin {margin:.3e}")
    assert len(masses) == so.GRAPH_STEPS and margin >= so.MARGIN, margin
