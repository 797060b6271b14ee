"""Vanilla resamplers on MI355X: afldm_conv2d_s2 / afldm_conv2d_up2 against F.conv2d on the CPU at every FFHQ-UNet and
VAE site, and the vanilla models built with af_api.enable_vanilla_resampling (tiny UNet forward + taps vs the committed
oracle fixture, 50 DDIM steps graph / eager, the shift harness, tiny VAEs, the FFHQ-size UNet) against the CPU oracle.
Tolerances: relative RMS 1e-4 fp32 / 2e-2 bf16 for a forward pass."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
FWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}


def rel_rms(got, ref):
    got, ref = got.double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def nchw(y):
    return y.float().permute(0, 3, 1, 2)


# (Cin = Cout, input plane) of every site; the UNet is FFHQ_UNET (sample 32), the VAE the AF-VAE config at 256^2
S2_SITES = [("unet", 192, 32), ("unet", 384, 16), ("unet", 384, 8), ("unet", 768, 4),
            ("vae", 128, 256), ("vae", 256, 128), ("vae", 512, 64)]
UP2_SITES = [("unet", 768, 2), ("unet", 768, 4), ("unet", 384, 8), ("unet", 384, 16),
             ("vae", 512, 32), ("vae", 512, 64), ("vae", 256, 128)]
CHECK = (0, 33, 63)          # samples compared on the CPU at B = 64 (the GPU computes all of them)


def _operands(C, N, B, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)
    b = torch.randn(C, generator=g) * 0.1
    if dtype == torch.bfloat16:
        w = w.to(dtype).float()
    x = torch.empty(B, N, N, C, device="cuda")
    x.normal_(generator=torch.Generator(device="cuda").manual_seed(seed))
    return x.to(dtype), w, b


def _check_stats(y):
    """The statistics the epilogue wrote equal a stand-alone afldm_gn_stats pass over the result (per-channel totals)."""
    from afldm_amd import ops
    ref = ops.gn_stats(y.clone()).st1
    s, r = y.gn_partial.double().sum(1).cpu(), ref.double().sum(1).cpu()
    scale = r.abs().amax(1, keepdim=True) + 1.0
    assert float(((s - r).abs() / scale).max()) <= 1e-4


def _run_site(kind, C, N, B, dtype, op, pad=(1, 1)):
    from afldm_amd import ops
    x, w, b = _operands(C, N, B, dtype, seed=C + N + B)
    xd, bd = x, b.cuda()
    if op == "s2":
        y = ops.conv2d_s2(xd, ops.pack_weight(w.cuda(), dtype), bd, pad=pad, want_stats=True)
    else:
        y = ops.conv2d_up2(xd, ops.pack_weight_up2(w.cuda(), dtype), bd, want_stats=True)
    torch.cuda.synchronize()
    idx = list(range(B)) if B <= 2 else list(CHECK)
    xs = x[idx].float().cpu().permute(0, 3, 1, 2)
    if op == "s2":
        ref = F.conv2d(F.pad(xs, (pad[0], pad[1], pad[0], pad[1])), w, b, stride=2)
    else:
        ref = F.conv2d(F.interpolate(xs, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    got = nchw(y[idx].cpu())
    r = rel_rms(got, ref)
    assert r <= FWD_TOL[dtype], (kind, C, N, B, r)
    _check_stats(y)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("site", S2_SITES, ids=lambda s: f"{s[0]}{s[1]}x{s[2]}")
def test_conv2d_s2_sites(site, B, dtype):
    kind, C, N = site
    _run_site(kind, C, N, B, dtype, "s2", pad=(1, 1) if kind == "unet" else (0, 1))


@pytest.mark.parametrize("pad", [(1, 1), (0, 1)])
def test_conv2d_s2_both_paddings_small(pad):
    _run_site("unet", 64, 16, 2, torch.float32, "s2", pad=pad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("site", UP2_SITES, ids=lambda s: f"{s[0]}{s[1]}x{s[2]}")
def test_conv2d_up2_sites(site, B, dtype):
    kind, C, N = site
    _run_site(kind, C, N, B, dtype, "up2")


def test_pack_weight_up2_matches_host_fold():
    from afldm_amd import ops
    w = torch.randn(64, 72, 3, 3, generator=torch.Generator().manual_seed(5))
    got = ops.pack_weight_up2(w.cuda(), torch.float32).cpu()               # [4, Cout, 2, 2, Cin]
    want = ops.fold_up2_weight(w).permute(0, 1, 3, 4, 2)
    assert torch.equal(got, want)
    got16 = ops.pack_weight_up2(w.cuda(), torch.bfloat16).cpu()
    assert torch.equal(got16, want.to(torch.bfloat16))


def test_conv2d_up2_input_over_2gib():
    """The VAE decoder's 128^2 -> 256^2 site with an input of more than 2 GiB (fp32, 130 samples: two launches of 65)."""
    from afldm_amd import ops
    C, N, B = 256, 128, 130
    g = torch.Generator().manual_seed(7)
    w = torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)
    b = torch.randn(C, generator=g) * 0.1
    x = torch.empty(B, N, N, C, device="cuda")
    x.normal_(generator=torch.Generator(device="cuda").manual_seed(3))
    assert x.numel() * 4 > 2 ** 31
    y = ops.conv2d_up2(x, ops.pack_weight_up2(w.cuda(), torch.float32), b.cuda(), want_stats=True)
    torch.cuda.synchronize()
    idx = [0, 64, 65, 129]
    xs = x[idx].cpu().permute(0, 3, 1, 2)
    ref = F.conv2d(F.interpolate(xs, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    assert rel_rms(nchw(y[idx].cpu()), ref) <= 1e-4
    st = y.gn_partial.double().sum(1)[idx].cpu()
    r = ref.double()
    want = torch.stack([r.sum((2, 3)), r.pow(2).sum((2, 3))], -1)
    assert float(((st - want).abs() / (want.abs() + 1.0)).max()) <= 1e-3


# ----------------------------------------------------------------------------- vanilla models
def build_unet(cfg_name, dtype):
    from afldm_amd.af_modules.af_api import enable_vanilla_resampling
    from afldm_amd.models.unet_2d import UNet2DModel
    from oracle import configs as oc, unet as ou
    if cfg_name == "tiny":
        cfg = oc.tiny_unet()
        sd = ou.randomize_norm_affine(ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1))
    else:
        cfg = oc.FFHQ_UNET
        sd = ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1)
    unet = UNet2DModel.from_config(cfg)
    unet.load_state_dict(sd)
    enable_vanilla_resampling(unet)
    return unet.to("cuda").to(dtype), cfg, sd


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tiny_vanilla_unet_forward_and_taps(golden, dtype):
    g = golden("g6_tiny_unet.npz")
    unet, cfg, _ = build_unet("tiny", dtype)
    taps = {}
    names = ["down_blocks.0.resnets.0", "down_blocks.0.attentions.0", "down_blocks.0.downsamplers.0",
             "mid_block.resnets.1", "up_blocks.0.upsamplers.0", "up_blocks.2.attentions.1"]
    mods = dict(unet.named_modules())
    hooks = [mods[n].register_forward_hook(lambda m, i, o, n=n: taps.__setitem__(n, o)) for n in names]
    x = torch.from_numpy(g["x"]).cuda()
    y = unet(x, 501, return_dict=False)[0]
    for h in hooks:
        h.remove()
    for n in names:
        r = rel_rms(nchw(taps[n]), g[f"tap_vanilla:{n}"])
        assert r <= FWD_TOL[dtype], (n, r)
    assert rel_rms(y, g["y_vanilla"]) <= FWD_TOL[dtype]


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 5e-2)])
def test_vanilla_ddim_50_steps_graph_and_eager(golden, dtype, tol):
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from oracle import pipeline as op
    g = golden("g6_tiny_unet.npz")
    unet, cfg, sd = build_unet("tiny", dtype)
    x = torch.from_numpy(g["x"])
    want = op.ddim_sample(sd, cfg, x, 50, af=False)
    eng = DenoiseEngine(unet, ffhq_ddim_scheduler(), 2, 50, use_graph=True)
    eng.reset(x)
    eng.step(50)
    out_graph = eng.lat.clone()
    assert rel_rms(out_graph, want) <= tol
    eager = DenoiseEngine(unet, ffhq_ddim_scheduler(), 2, 50, use_graph=False).run(x)
    assert torch.equal(eager, out_graph), "graph replay must be bit-identical to eager launches"


def test_state_key_changes_when_resamplers_are_swapped():
    from afldm_amd.af_modules.af_api import enable_vanilla_resampling
    from afldm_amd.engine import model_state_key
    from afldm_amd.models.unet_2d import UNet2DModel
    from oracle import configs as oc
    unet = UNet2DModel.from_config(oc.tiny_unet()).cuda()
    k0 = model_state_key(unet)
    enable_vanilla_resampling(unet)
    k1 = model_state_key(unet)
    assert k1 != k0
    enable_vanilla_resampling(unet)
    assert model_state_key(unet) == k1


@pytest.mark.parametrize("dtype,db_tol", [(torch.float32, 0.2), (torch.bfloat16, 1.0)])
def test_vanilla_shift_equivariance_vs_oracle(dtype, db_tol):
    """Latent core of shift_ldm on the vanilla tiny UNet (cross-frame STORE pass, ideal-crop shifted LOAD passes, 4 DDIM
    steps) against oracle.pipeline.shift_equivariance(af=False) computed here."""
    from afldm_amd.pipelines.cross_frame_attn import (AttnState, CrossFrameAttnProcessor, get_unet_attn_processors,
                                                      set_unet_attn_processor)
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.shift_utils.metrics import mask_mse
    from afldm_amd.shift_utils.shifters import ImageShifter
    from oracle import pipeline as op
    unet, cfg, sd = build_unet("tiny", dtype)
    x = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(1234))
    base_ref, res_ref = op.shift_equivariance(sd, cfg, x, [0.375, 1.0], 4, ratio=8, af=False)
    state = AttnState()
    set_unet_attn_processor(unet, {k: CrossFrameAttnProcessor(state) for k in get_unet_attn_processors(unet)})
    sched = ffhq_ddim_scheduler()

    def denoise(z):
        sched.set_timesteps(4, device="cuda")
        for t in sched.timesteps:
            state.set_timestep(t)
            eps = unet(sched.scale_model_input(z, t), t, return_dict=False)[0]
            z = sched.step(eps, t, z, eta=0, return_dict=False)[0]
        return z

    xd = x.cuda()
    state.reset()
    base = denoise(xd)
    state.to_load()
    assert rel_rms(base, base_ref) <= (1e-3 if dtype == torch.float32 else 5e-2)
    for k, tj in enumerate((0.375, 1.0)):
        xs, mask = ImageShifter("ideal_crop", 8).shift(xd, 0, tj)
        den = denoise(xs)
        ref, _ = ImageShifter("ideal_crop", 8).shift(base, 0, tj)
        mse, want = float(mask_mse(den, ref, mask)), res_ref[k]["mse"]
        assert abs(10 * np.log10(mse / want)) <= db_tol, (tj, mse, want)


def build_vae(dtype, up_rescale=None, af=True):
    from afldm_amd.af_modules.af_api import enable_vanilla_resampling, make_af_vae_from_config
    from afldm_amd.models.vae import AutoencoderKL
    from oracle import vae as ov
    cfg = ov.tiny_vae() if up_rescale is None else ov.tiny_vae(up_rescale=up_rescale)
    sd = ov.init_vae_params(cfg, seed=3)
    vae = AutoencoderKL(in_channels=3, out_channels=3, down_block_types=["DownEncoderBlock2D"] * 4,
                        up_block_types=["UpDecoderBlock2D"] * 4, block_out_channels=cfg["block_out_channels"],
                        layers_per_block=cfg["layers_per_block"], latent_channels=4, norm_num_groups=32,
                        scaling_factor=cfg["scaling_factor"], mid_act=cfg["mid_act"],
                        down_filtered_act=cfg["down_filtered_act"], up_filtered_act=cfg["up_filtered_act"],
                        up_rescale=cfg["up_rescale"])
    vae.load_state_dict(sd)
    if af:
        make_af_vae_from_config(vae)
    enable_vanilla_resampling(vae)
    return vae.to("cuda").to(dtype), cfg, sd


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("variant", ["stock", "partly_af"])
def test_tiny_vanilla_vae_encode_decode(variant, dtype):
    from oracle import vae as ov
    if variant == "stock":
        vae, cfg, sd = build_vae(dtype, af=False)
        # the oracle of a model without alias-free surgery: every switch off
        cfg = dict(cfg, mid_act=False, down_filtered_act=[False] * 4, up_filtered_act=[False] * 4,
                   up_rescale=[False] * 3)
    else:
        vae, cfg, sd = build_vae(dtype, up_rescale=[True, False, True])
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    z = torch.randn(2, 4, 8, 8, generator=g)
    post = vae.encode(x.cuda()).latent_dist
    assert rel_rms(post.parameters, ov.encode_moments(sd, cfg, x)) <= FWD_TOL[dtype] * (1.5 if dtype == torch.bfloat16 else 1)
    img = vae.decode(z.cuda(), return_dict=False)[0]
    assert rel_rms(img, ov.decode(sd, cfg, z)) <= FWD_TOL[dtype] * (1.5 if dtype == torch.bfloat16 else 1)


def test_ffhq_vanilla_unet_forward_bf16():
    from oracle import unet as ou
    unet, cfg, sd = build_unet("ffhq", torch.bfloat16)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(21))
    y = unet(x.cuda(), 981, return_dict=False)[0]
    ref = ou.unet_forward(sd, cfg, x, 981, af=False)
    assert rel_rms(y, ref) <= 2e-2
