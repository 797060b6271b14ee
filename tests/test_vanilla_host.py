"""Vanilla resamplers, host side (no GPU): the nearest-x2 phase fold of afldm_conv2d_up2 as pure torch against the literal
upsample + convolution, and the module swap of af_api.enable_vanilla_resampling on a UNet, a partly alias-free VAE and a
stock VAE."""
import pytest
import torch
import torch.nn.functional as F


def _phase_conv(x, w, b):
    """conv3x3(nearest2x(x)) through the folded weights: four 2x2 convolutions of x, interleaved."""
    from afldm_amd.ops import fold_up2_weight
    wf = fold_up2_weight(w)                                   # [4, Cout, Cin, 2, 2]
    B, _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty(B, w.shape[0], 2 * H, 2 * W)
    for p in range(4):
        a, c = divmod(p, 2)
        y = F.conv2d(xp[:, :, a:a + H + 1, c:c + W + 1], wf[p], b)
        out[:, :, a::2, c::2] = y
    return out


@pytest.mark.parametrize("N", [2, 4, 16])
def test_phase_fold_equals_nearest_upsample_conv(N):
    g = torch.Generator().manual_seed(N)
    x = torch.randn(2, 24, N, N, generator=g)
    w = torch.randn(40, 24, 3, 3, generator=g) / 15
    b = torch.randn(40, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    got = _phase_conv(x, w, b)
    assert float((got - ref).norm() / ref.norm()) <= 1e-6


def test_phase_fold_layout_and_sums():
    from afldm_amd.ops import fold_up2_weight
    w = torch.randn(3, 5, 3, 3, dtype=torch.float64).float()
    wf = fold_up2_weight(w)
    assert wf.shape == (4, 3, 5, 2, 2) and wf.dtype == torch.float32
    # every phase sums all nine taps once
    assert torch.allclose(wf.sum((3, 4)), w.sum((2, 3)).expand(4, 3, 5), atol=1e-5)
    assert torch.equal(wf[0, :, :, 0, 0], w[:, :, 0, 0])      # phase (0, 0), tap (i-1, j-1): w0 x w0
    assert torch.equal(wf[3, :, :, 1, 1], w[:, :, 2, 2])      # phase (1, 1), tap (i+1, j+1): w2 x w2


def _tiny_unet():
    from afldm_amd.models.unet_2d import UNet2DModel
    from oracle import configs as oc
    return UNet2DModel.from_config(oc.tiny_unet())


def _vae(up_rescale=None):
    from afldm_amd.models.vae import AutoencoderKL
    from oracle import vae as ov
    cfg = ov.tiny_vae() if up_rescale is None else ov.tiny_vae(up_rescale=up_rescale)
    return AutoencoderKL(in_channels=3, out_channels=3, down_block_types=["DownEncoderBlock2D"] * 4,
                         up_block_types=["UpDecoderBlock2D"] * 4, block_out_channels=cfg["block_out_channels"],
                         layers_per_block=cfg["layers_per_block"], latent_channels=4, norm_num_groups=32,
                         scaling_factor=cfg["scaling_factor"], mid_act=cfg["mid_act"],
                         down_filtered_act=cfg["down_filtered_act"], up_filtered_act=cfg["up_filtered_act"],
                         up_rescale=cfg["up_rescale"])


def _samplers(model):
    from afldm_amd.models.blocks import Downsample2D, Upsample2D
    return {n: m for n, m in model.named_modules() if isinstance(m, (Downsample2D, Upsample2D))}


def _check_swap(model, expect_vanilla):
    """Swap, then: exactly the names in expect_vanilla became HIP vanilla modules sharing the original conv, everything
    else is the same object, state-dict keys and tensors are unchanged, and a second call is a no-op."""
    from afldm_amd.af_modules.af_api import enable_vanilla_resampling
    from afldm_amd.models.blocks import NearestUpsample2D, StridedDownsample2D
    before = _samplers(model)
    sd_before = model.state_dict()
    convs = {n: m.conv for n, m in before.items()}
    assert enable_vanilla_resampling(model) is model
    after = _samplers(model)
    assert set(after) == set(before)
    for n, m in after.items():
        if n in expect_vanilla:
            assert type(m) is (StridedDownsample2D if "down" in n else NearestUpsample2D), n
            assert m.conv is convs[n] and m is not before[n], n
            assert (m.channels, m.out_channels, m.use_conv, m.name) == (before[n].channels, before[n].out_channels,
                                                                       before[n].use_conv, before[n].name)
        else:
            assert m is before[n], n
    sd_after = model.state_dict()
    assert list(sd_after) == list(sd_before)
    assert all(sd_after[k] is sd_before[k] or sd_after[k].data_ptr() == sd_before[k].data_ptr() for k in sd_before)
    again = dict(_samplers(model))
    enable_vanilla_resampling(model)
    assert all(_samplers(model)[n] is m for n, m in again.items())


def test_enable_vanilla_resampling_on_unet():
    unet = _tiny_unet()
    names = set(_samplers(unet))
    assert names == {"down_blocks.0.downsamplers.0", "down_blocks.1.downsamplers.0", "up_blocks.0.upsamplers.0",
                     "up_blocks.1.upsamplers.0"}
    _check_swap(unet, names)
    assert unet.down_blocks[0].downsamplers[0].padding == 1


def test_enable_vanilla_resampling_on_partly_alias_free_vae():
    from afldm_amd.af_modules.af_api import make_af_vae_from_config
    from afldm_amd.af_modules.af_blocks import AliasFreeDownsample2D, AliasFreeUpsample2D
    vae = _vae(up_rescale=[True, False, True])
    make_af_vae_from_config(vae)
    # decoder level 1 keeps its vanilla upsampler; the encoder pairs level i with decoder level (2 - i): level 1 again
    assert type(vae.decoder.up_blocks[1].upsamplers[0]).__name__ == "Upsample2D"
    assert type(vae.encoder.down_blocks[1].downsamplers[0]).__name__ == "Downsample2D"
    assert isinstance(vae.decoder.up_blocks[0].upsamplers[0], AliasFreeUpsample2D)
    assert isinstance(vae.encoder.down_blocks[0].downsamplers[0], AliasFreeDownsample2D)
    _check_swap(vae, {"encoder.down_blocks.1.downsamplers.0", "decoder.up_blocks.1.upsamplers.0"})
    assert vae.encoder.down_blocks[1].downsamplers[0].padding == 0


def test_enable_vanilla_resampling_on_stock_vae():
    vae = _vae()
    names = set(_samplers(vae))
    assert len(names) == 6
    _check_swap(vae, names)


def test_unet_without_opt_in_still_raises():
    from afldm_amd.models.blocks import Downsample2D, Upsample2D
    unet = _tiny_unet()
    x = torch.zeros(1, 16, 16, 64)
    with pytest.raises(NotImplementedError, match="make_af_unet") as e:
        unet.down_blocks[0].downsamplers[0](x)
    assert "enable_vanilla_resampling" in str(e.value)
    with pytest.raises(NotImplementedError, match="make_af_unet") as e:
        Upsample2D(64, use_conv=True)(x)
    assert "enable_vanilla_resampling" in str(e.value)
    assert type(unet.down_blocks[0].downsamplers[0]) is Downsample2D


def test_opt_in_is_exported_under_both_import_paths():
    import afldm.af_modules.af_api as a
    import afldm_amd.af_modules.af_api as b
    assert a.enable_vanilla_resampling is b.enable_vanilla_resampling
    assert "enable_vanilla_resampling" in b.__all__
