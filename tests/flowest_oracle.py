"""CPU oracle of the built-in optical-flow estimator (afldm_amd/shift_utils/flow_estimation.py, csrc/flowest.hip): dense
pyramidal Lucas-Kanade with Tikhonov damping and iterative warping, written in torch, dtype-generic (run it in float64 for the
reference value and in float32 for the rounding scale delta = max |fp32 - fp64| the GPU tests are held to).

This is NOT the reference's GMFlow (a trained network whose weights are not available): it is a classical, deterministic
estimator this project defines, and this file is its specification.  Every operation is continuous in its inputs (replicate
borders, clamped sampling coordinates, no validity mask), so the float32 run stays next to the float64 run.  Every sum is
spelled term by term in a fixed order, each product and each add a rounded operation of its own, so that a kernel can restate
it.  Flows are [B, 2, H, W] with channel 0 = ROW displacement."""
import math

import torch

DOWN_TAPS = (0.125, 0.375, 0.375, 0.125)                    # [1, 3, 3, 1] / 8
SMOOTH_TAPS = (0.0625, 0.25, 0.375, 0.25, 0.0625)           # [1, 4, 6, 4, 1] / 16


def _taps_along(x, dim, index_rows, taps):
    """sum_k taps[k] * x.index_select(dim, index_rows[k]), added left to right."""
    acc = None
    for w, idx in zip(taps, index_rows):
        term = x.index_select(dim, idx) * w
        acc = term if acc is None else acc + term
    return acc


def pyr_down(x):
    """[..., H, W] -> [..., H/2, W/2]: [1, 3, 3, 1] / 8 along the columns, then along the rows, decimated by 2; output (y, x)
    reads rows 2y-1 .. 2y+2 and columns 2x-1 .. 2x+2, indices clamped into the plane."""
    H, W = x.shape[-2:]
    cols = [(2 * torch.arange(W // 2) - 1 + k).clamp(0, W - 1) for k in range(4)]
    rows = [(2 * torch.arange(H // 2) - 1 + k).clamp(0, H - 1) for k in range(4)]
    return _taps_along(_taps_along(x, -1, cols, DOWN_TAPS), -2, rows, DOWN_TAPS)


def pyramid(x, levels):
    out = [x]
    for _ in range(levels - 1):
        out.append(pyr_down(out[-1]))
    return out


def smooth(u):
    """[1, 4, 6, 4, 1] / 16 along the columns, then along the rows, replicate border."""
    H, W = u.shape[-2:]
    cols = [(torch.arange(W) - 2 + k).clamp(0, W - 1) for k in range(5)]
    rows = [(torch.arange(H) - 2 + k).clamp(0, H - 1) for k in range(5)]
    return _taps_along(_taps_along(u, -1, cols, SMOOTH_TAPS), -2, rows, SMOOTH_TAPS)


def _bilinear(planes, sy, sx):
    """planes [B, C, h, w] at the (already clamped) coordinates sy, sx [B, H, W]: (1 - fy) ((1 - fx) v00 + fx v01) + fy (...)."""
    B, C, h, w = planes.shape
    y0f, x0f = torch.floor(sy), torch.floor(sx)
    fy, fx = (sy - y0f)[:, None], (sx - x0f)[:, None]
    y0, x0 = y0f.long(), x0f.long()
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
    flat = planes.reshape(B, C, h * w)

    def at(yy, xx):
        idx = (yy * w + xx).reshape(B, 1, -1).expand(B, C, -1)
        return torch.gather(flat, 2, idx).reshape(B, C, *sy.shape[1:])

    top = (1 - fx) * at(y0, x0) + fx * at(y0, x1)
    bot = (1 - fx) * at(y1, x0) + fx * at(y1, x1)
    return (1 - fy) * top + fy * bot


def up2(u):
    """Step 2: 2 * bilinear_up2(u), half-pixel centres: source coordinate (y + 0.5) / 2 - 0.5 clamped to [0, h - 1]."""
    B, _, h, w = u.shape
    sy = ((torch.arange(2 * h, dtype=u.dtype) + 0.5) / 2 - 0.5).clamp(0, h - 1)
    sx = ((torch.arange(2 * w, dtype=u.dtype) + 0.5) / 2 - 0.5).clamp(0, w - 1)
    sy = sy[None, :, None].expand(B, 2 * h, 2 * w)
    sx = sx[None, None, :].expand(B, 2 * h, 2 * w)
    return _bilinear(u, sy, sx) * 2


def warp(I2, u):
    """I2w(p) = bilinear(I2, clamp(p + u(p)))."""
    B, _, H, W = I2.shape
    yy = torch.arange(H, dtype=u.dtype)[None, :, None]
    xx = torch.arange(W, dtype=u.dtype)[None, None, :]
    return _bilinear(I2, (yy + u[:, 0]).clamp(0, H - 1), (xx + u[:, 1]).clamp(0, W - 1))


def _shift(x, dim, d):
    n = x.shape[dim]
    return x.index_select(dim, (torch.arange(n) + d).clamp(0, n - 1))


def _box(x, r):
    """Sum over the (2r + 1)^2 window, replicate-padded: along the columns left to right, then along the rows top to bottom."""
    for dim in (-1, -2):
        acc = _shift(x, dim, -r)
        for d in range(-r + 1, r + 1):
            acc = acc + _shift(x, dim, d)
        x = acc
    return x


def lk_step(I1, I2, u, radius=3, lam=1e-3):
    """Step 3: one damped Lucas-Kanade update of u [B, 2, H, W] for the pair I1, I2 [B, C, H, W]."""
    I2w = warp(I2, u)
    d1y = (_shift(I1, -2, 1) - _shift(I1, -2, -1)) * 0.5
    d1x = (_shift(I1, -1, 1) - _shift(I1, -1, -1)) * 0.5
    d2y = (_shift(I2w, -2, 1) - _shift(I2w, -2, -1)) * 0.5
    d2x = (_shift(I2w, -1, 1) - _shift(I2w, -1, -1)) * 0.5
    gy, gx = (d1y + d2y) * 0.5, (d1x + d2x) * 0.5
    It = I2w - I1

    def csum(t):                                            # over the channels, in order
        acc = t[:, 0]
        for c in range(1, t.shape[1]):
            acc = acc + t[:, c]
        return acc

    n = float((2 * radius + 1) ** 2)
    a, b, c, p, q = (_box(csum(t), radius) / n for t in (gy * gy, gy * gx, gx * gx, gy * It, gx * It))
    a, c = a + lam, c + lam
    det = a * c - b * b
    du0 = -((c * p - b * q) / det)
    du1 = -((a * q - b * p) / det)
    s = (1 / torch.sqrt(du0 * du0 + du1 * du1)).clamp(max=1)            # 1 / 0 = inf -> 1
    return torch.stack([u[:, 0] + du0 * s, u[:, 1] + du1 * s], 1)


def default_levels(H, W):
    return int(math.log2(min(H, W))) - 2


def estimate(I1, I2, levels=None, iters=3, radius=3, lam=1e-3):
    """The flow u [B, 2, H, W] with I2(p + u(p)) ~ I1(p)."""
    H, W = I1.shape[-2:]
    levels = default_levels(H, W) if levels is None else levels
    if levels < 1 or H % (1 << (levels - 1)) or W % (1 << (levels - 1)):
        raise ValueError(f"H = {H} and W = {W} must be divisible by 2^(levels - 1) = {1 << max(levels - 1, 0)}")
    p1, p2 = pyramid(I1, levels), pyramid(I2, levels)
    u = torch.zeros(I1.shape[0], 2, *p1[-1].shape[-2:], dtype=I1.dtype)
    for l in range(levels - 1, -1, -1):
        if l < levels - 1:
            u = up2(u)
        for _ in range(iters):
            u = smooth(lk_step(p1[l], p2[l], u, radius, lam))
    return u


def bidirectional(image1, image2, **kw):
    """(fwd, bwd), each [N, 2, H, W], from one batched run over (I1 -> I2, I2 -> I1)."""
    N = image1.shape[0]
    u = estimate(torch.cat([image1, image2]), torch.cat([image2, image1]), **kw)
    return u[:N], u[N:]


# ------------------------------------------------------------------------------------------------- test inputs
def texture(seed, S, channels=3, Sw=None):
    """torch.manual_seed(seed); randn(1, channels, S, Sw) in float64, ideal low-pass keeping |f| <= 0.2 cycles / pixel on both
    axes, divided by max |x|."""
    Sw = S if Sw is None else Sw
    torch.manual_seed(seed)
    x = torch.randn(1, channels, S, Sw, dtype=torch.float64)
    keep = (torch.fft.fftfreq(S).abs() <= 0.2)[:, None] & (torch.fft.fftfreq(Sw).abs() <= 0.2)[None, :]
    x = torch.fft.ifft2(torch.fft.fft2(x) * keep).real
    return x / x.abs().max()


def translate(x, dy, dx):
    """The periodic translation x(. - (dy, dx)) by the Fourier phase shift: I2 = translate(I1, d) has the flow u = d."""
    H, W = x.shape[-2:]
    ph = torch.exp(-2j * math.pi * (torch.fft.fftfreq(H, dtype=torch.float64)[:, None] * dy +
                                    torch.fft.fftfreq(W, dtype=torch.float64)[None, :] * dx))
    return torch.fft.ifft2(torch.fft.fft2(x) * ph).real


def patch_pair(S=64, box=(16, 20, 24), move=(5, -3), seeds=(1, 2)):
    """(I1, I2): a box[2]^2 patch of a second texture at (box[0], box[1]) of I1 moved by `move` in I2, over a static
    background texture."""
    bg, fg = texture(seeds[0], S), texture(seeds[1], S)
    y, x, n = box
    I1, I2 = bg.clone(), bg.clone()
    I1[..., y:y + n, x:x + n] = fg[..., y:y + n, x:x + n]
    I2[..., y + move[0]:y + move[0] + n, x + move[1]:x + move[1] + n] = fg[..., y:y + n, x:x + n]
    return I1, I2


def smooth_field(seed, B, H, W, amp):
    """A smooth random flow field [B, 2, H, W] (float64) scaled to max |u| = amp: half a smooth random field, half an outward
    ramp, so that samples are pushed across all four borders."""
    torch.manual_seed(seed)
    z = torch.randn(B, 2, max(H // 8, 2), max(W // 8, 2), dtype=torch.float64)
    u = torch.nn.functional.interpolate(z, size=(H, W), mode="bicubic", align_corners=True)
    out = torch.stack(torch.meshgrid(torch.linspace(-1, 1, H, dtype=torch.float64), torch.linspace(-1, 1, W, dtype=torch.float64),
                                     indexing="ij"))[None]
    u = u / u.abs().max() + out
    return u / u.abs().max() * amp


def median_epe(u, want, region):
    """Median end-point error of u [2, H, W] against the constant displacement `want` over the slices `region`."""
    ys, xs = region
    e = torch.sqrt((u[0, ys, xs] - want[0]) ** 2 + (u[1, ys, xs] - want[1]) ** 2)
    return float(e.median())
