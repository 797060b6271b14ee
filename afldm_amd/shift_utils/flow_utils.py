"""Warping along an optical-flow field on MI355X — the part of the reference's afldm/shift_utils/flow_utils.py and
flow_utils_np.py that needs no flow MODEL, with its signatures:

  coords_grid, bilinear_sample, flow_warp (:35-86)                 -> afldm_flow_warp (grid_sample, align_corners=True, zeros)
  flow_warp_with_occ_bg (:89-114)                                   -> flow_warp / apply_fractional_translation + the fill
  forward_backward_consistency_check (:135-157), get_patch_moving_flow (:242-259)
  forward_flow_warp (flow_utils_np.py:107-160), forward_upsample_flow_warp (:333-341),
  continuous_noise_fwd_warp (:262-267)                              -> afldm_flow_splat (pick / pool mode)
  upsample_noise (:205-211), collect_noise_pixel (:214-221)
  forward_flow_warp_frames: every frame of one endpoint in one afldm_flow_splat call (the image-interpolation pipeline's entry)

Flow tensors are fp32 [B, 2, H, W] with channel 0 = ROW displacement wherever the reference's are (flow_warp flips them
itself).  Where the reference draws from the global RNG, the functions here take keyword-only `generator` (drawn with
utils.randn_tensor: a CPU generator draws on the CPU and moves the tensor) and `noise` (the draw itself, e.g. an oracle's;
`noise_draw` in upsample_noise and collect_noise_pixel, whose first argument already has that name).
Device tensors only: CPU tensors raise.  Absent: everything that calls a flow model (predict_flow,
get_warped_and_mask, alpha_warp, InputPadder), the rounding scatter / gather family (flow_warp2, flow_revserse_map,
get_intermediate_warp_mask, continuous_noise_warp, continuous_noise_warp_bwd) and the training-time random translations.
Coordinates stay in fp32 for bf16 images (the reference rounds the sampling grid to the image's dtype)."""
import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..utils import randn_tensor


def _f32(t):
    return t.float().contiguous()


def _scales(alpha, n, device):
    """fp32 [n] device tensor of the factor the reference multiplies the flow by (a Python float is rounded to fp32 there)."""
    if torch.is_tensor(alpha):
        return alpha.detach().to(device=device, dtype=torch.float32).reshape(-1).expand(n).contiguous()
    return torch.full((n,), float(alpha), dtype=torch.float32, device=device)


def _draw(like, generator, noise):
    if noise is not None:
        if tuple(noise.shape) != tuple(like.shape):
            raise ValueError(f"noise must have the shape of the draw it replaces, {tuple(like.shape)}, got {tuple(noise.shape)}")
        return noise.to(device=like.device, dtype=like.dtype).contiguous()
    return randn_tensor(tuple(like.shape), generator=generator, device=like.device, dtype=like.dtype)


def coords_grid(b, h, w, homogeneous=False, device=None):
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    stacks = [x, y] + ([torch.ones_like(x)] if homogeneous else [])
    grid = torch.stack(stacks, dim=0).float()[None].repeat(b, 1, 1, 1)
    return grid if device is None else grid.to(device)


def _sampler_mode(mode, padding_mode):
    if mode not in ("bilinear", "nearest"):
        raise NotImplementedError(f"mode={mode!r}: afldm_flow_warp samples 'bilinear' and 'nearest'")
    if padding_mode != "zeros":
        raise NotImplementedError(f"padding_mode={padding_mode!r}: afldm_flow_warp pads with zeros")
    return mode == "nearest"


def bilinear_sample(img, sample_coords, mode="bilinear", padding_mode="zeros", return_mask=False):
    """img [B, C, H, W] sampled at sample_coords [B, 2, h, w] (or [B, h, w, 2]) in pixels, channel 0 = x."""
    nearest = _sampler_mode(mode, padding_mode)
    if sample_coords.size(1) != 2:
        sample_coords = sample_coords.permute(0, 3, 1, 2)
    return ops.flow_warp(img.contiguous(), _f32(sample_coords), add_grid=False, nearest=nearest, mask=return_mask)


def flow_warp(feature, flow, mask=False, mode="bilinear", padding_mode="zeros"):
    """feature [B, C, H, W] sampled at (i + flow[:, 0], j + flow[:, 1]): the reference's coords_grid + flip(flow)."""
    nearest = _sampler_mode(mode, padding_mode)
    assert flow.size(1) == 2
    return ops.flow_warp(feature.contiguous(), _f32(flow), add_grid=True, nearest=nearest, mask=mask)


def flow_warp_with_occ_bg(img, flow, mask, is_randn, filter=None, *, generator=None, noise=None):
    """filter choices: [None, 'lanczos'].  noise: the background itself ([n, c, h, w] for is_randn, else [n, c, 1, 1])."""
    if not img.is_cuda:
        raise RuntimeError("afldm_amd: img must live on an MI355X (cuda) device; there is no CPU path")
    if is_randn:
        background = _draw(img, generator, noise)
    else:
        n, c = img.shape[0:2]
        if noise is None:            # drawn where the generator lives (the CPU without one, as the reference), then moved
            gdev = generator.device if generator is not None else "cpu"
            background = torch.rand((n, c, 1, 1), generator=generator, device=gdev) * 2 - 1
        else:
            background = noise
        background = background.to(device=img.device, dtype=img.dtype)
    if filter == "lanczos":
        from ..af_libs.equivariance import apply_fractional_translation
        _, _, h, w = img.shape
        tx = -flow[0, 1, 0, 0].item() / w
        ty = -flow[0, 0, 0, 0].item() / h
        warped_img, _ = apply_fractional_translation(img, tx, ty)
    elif filter is None:
        warped_img = flow_warp(img, flow)
    else:
        raise ValueError(f"filter must be None or 'lanczos', got {filter!r}")
    return warped_img * mask + background * (1 - mask)


def forward_backward_consistency_check(fwd_flow, bwd_flow, alpha=0.01, beta=0.5):
    """UnFlow's check (https://arxiv.org/abs/1711.07837): (fwd_occ, bwd_occ), each fp32 [B, 1, H, W]."""
    assert fwd_flow.dim() == 4 and bwd_flow.dim() == 4
    assert fwd_flow.size(1) == 2 and bwd_flow.size(1) == 2
    flow_mag = torch.norm(fwd_flow, dim=1) + torch.norm(bwd_flow, dim=1)
    warped_bwd_flow = flow_warp(bwd_flow, fwd_flow)
    warped_fwd_flow = flow_warp(fwd_flow, bwd_flow)
    diff_fwd = torch.norm(fwd_flow + warped_bwd_flow, dim=1)
    diff_bwd = torch.norm(bwd_flow + warped_fwd_flow, dim=1)
    threshold = alpha * flow_mag + beta
    return (diff_fwd > threshold).float().unsqueeze(1), (diff_bwd > threshold).float().unsqueeze(1)


def get_patch_moving_flow(img_template, region_box, displacement, alpha=1):
    """(bwd_flow, bwd_occ) of a patch region_box = (u, d, l, r) moved by alpha * displacement = (di, dj)."""
    n, _, h, w = img_template.shape
    u, d, l, r = region_box
    di, dj = displacement
    bwd_flow = torch.zeros(n, 2, h, w, device=img_template.device, dtype=torch.float32)
    bwd_occ = torch.zeros(n, 1, h, w, device=img_template.device, dtype=torch.float32)
    bwd_occ[:, :, u:d, l:r] = 1
    u, d = int(np.round(u + di * alpha)), int(np.round(d + di * alpha))
    l, r = int(np.round(l + dj * alpha)), int(np.round(r + dj * alpha))
    bwd_flow[:, 0, u:d, l:r] = -di * alpha
    bwd_flow[:, 1, u:d, l:r] = -dj * alpha
    bwd_occ[:, :, u:d, l:r] = 0
    return bwd_flow, bwd_occ


def forward_flow_warp(img, fwd_flow):
    """Forward bilinear splat of img [B, C, H, W] along fwd_flow [B, 2, H, W] (flow_utils_np.py:107-160): (warped, bwd_occ)
    with bwd_occ [B, 1, H, W] = 1 where no (net positive) weight landed; the sums are not divided by the weight."""
    img = img.contiguous()
    return ops.flow_splat(img, _f32(fwd_flow), _scales(1.0, img.shape[0], img.device))


def forward_flow_warp_frames(img, fwd_flow, alphas, ds=1, pool=False, fill=None, workspace=None):
    """The batched entry: img [Bs, C, H, W] warped along alphas[b] * fwd_flow [Bs, 2, H, W] for every b in one
    afldm_flow_splat call (alphas: fp32 device tensor [B] or a list of floats; sample b reads source b // (B // Bs)).
      pool=False: (warped[:, :, ::ds, ::ds], occ[:, :, ::ds, ::ds]); fill [1 | B, C, H, W] (full resolution, read at the kept
        pixels) applies warped * (1 - occ) + occ * fill, the image-interpolation pipeline's (:574).
      pool=True: (collect_noise_pixel(warped, occ, ds) with fill [1 | B, C, H, W] in place of its draw, occ at full resolution)."""
    img = img.contiguous()
    if not torch.is_tensor(alphas):
        alphas = torch.tensor([float(a) for a in alphas], dtype=torch.float32)
    alphas = alphas.to(device=img.device, dtype=torch.float32).reshape(-1).contiguous()
    return ops.flow_splat(img, _f32(fwd_flow), alphas, ds=ds, mode=ops.FLOW_POOL if pool else ops.FLOW_PICK,
                          fill=None if fill is None else fill.contiguous(), fill_pix_stride=ds, workspace=workspace)


def forward_upsample_flow_warp(img, fwd_flow, scale=8):
    """Ideal up-sampling by `scale`, forward warp at the high resolution, every scale-th pixel kept (:333-341); only the
    kept targets are accumulated."""
    from ..af_libs.ideal_lpf import UpsampleRFFT
    img = UpsampleRFFT(scale)(img)
    return forward_flow_warp_frames(img, fwd_flow, _scales(1.0, img.shape[0], img.device), ds=scale)


def upsample_noise(noise, ratio, *, generator=None, noise_draw=None):
    """Conditional up-sampling of white noise (:205-211): every low-resolution pixel is split into ratio x ratio unit-variance
    pixels whose sum / ratio is the pixel again."""
    if not noise.is_cuda:
        raise RuntimeError("afldm_amd: noise must live on an MI355X (cuda) device; there is no CPU path")
    n, c, h, w = noise.shape
    z = _draw(torch.empty(n, c, ratio * h, ratio * w, dtype=noise.dtype, device=noise.device), generator, noise_draw)
    z_mean = z.unfold(2, ratio, ratio).unfold(3, ratio, ratio).mean((4, 5))
    z_mean = F.interpolate(z_mean, scale_factor=ratio, mode="nearest")
    x = F.interpolate(noise, scale_factor=ratio, mode="nearest")
    return x / ratio + z - z_mean


def collect_noise_pixel(noise, bwd_occ, sidelength, *, generator=None, noise_draw=None):
    """(:214-221) occluded pixels take a fresh draw, then every sidelength x sidelength block is summed / sidelength."""
    if not noise.is_cuda:
        raise RuntimeError("afldm_amd: noise must live on an MI355X (cuda) device; there is no CPU path")
    sl = sidelength
    n, c, h, w = noise.shape
    res = _draw(noise, generator, noise_draw) * bwd_occ + noise * (1 - bwd_occ)
    res = res.reshape(n, c, h // sl, sl, w // sl, sl).permute(0, 1, 2, 4, 3, 5)
    return torch.sum(res, dim=(-1, -2)) / sidelength


def continuous_noise_fwd_warp(high_res_noise, fwd_flow, alpha, noise_ratio=8, *, generator=None, noise=None):
    """forward_flow_warp along alpha * fwd_flow + collect_noise_pixel (:262-267) as one afldm_flow_splat call in pool mode."""
    x = high_res_noise.contiguous()
    fill = _draw(x, generator, noise)
    return ops.flow_splat(x, _f32(fwd_flow), _scales(alpha, x.shape[0], x.device), ds=noise_ratio, mode=ops.FLOW_POOL, fill=fill)[0]
