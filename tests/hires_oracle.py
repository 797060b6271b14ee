"""High-resolution sampling (local + dilated windows, after DemoFusion) restated in torch on the CPU, float64 unless told otherwise,
on top of tests/pano_oracle.py (crop, fuse, x0_windows): the yardstick of csrc/hires.hip (afldm_hires_step, afldm_hires_windows) and
of MyLDMPipeline.hires_latents.  Not a test module.

A canvas [P, C, Hc, Hc] with Hc = scale * S is seen through NW = nwin + scale^2 windows per canvas, batch entry P * NW + k: the nwin
local windows of the geometry g (no wrap) in pano_oracle's order, then the dilated windows - window nwin + i * scale + j covers the
canvas elements (i + scale u, j + scale v).  The row is "hires"'s, (p, q, lo, hi, a, b, c, k0, k1, r, g, f):
    x0m = (1 - g) mean_k x0_k + g x0_g;  em = (1 - g) mean_k eps_k + g eps_g       (g == 0: the dilated eps is not looked at)
    xp  = a x0m + b em + c z                                                         (c == 0: z is not looked at)
    out = r (k0 ref + k1 eps_ref) + (1 - r) xp                                       (r == 0: ref / eps_ref are not looked at)
    next UNet input: the crops of out, and the sub-lattices of out + f (L out L^T - out)   (f == 0: L is not looked at)"""
import torch

import pano_oracle as po


def views(x, scale):
    """[P, C, Hc, Hc] -> [P, scale^2, C, S, S]: view i * scale + j is x[..., i::scale, j::scale].  Exact in any dtype."""
    return torch.stack([x[:, :, i::scale, j::scale] for i in range(scale) for j in range(scale)], 1)


def unviews(v, scale):
    """The inverse of views: [P, scale^2, C, S, S] -> [P, C, scale S, scale S]."""
    P, _, C, S, _ = v.shape
    x = torch.empty(P, C, scale * S, scale * S, dtype=v.dtype)
    for i in range(scale):
        for j in range(scale):
            x[:, :, i::scale, j::scale] = v[:, i * scale + j]
    return x


def split(windows, g, scale):
    """[P * NW, C, S, S] -> (local [P * nwin, C, S, S], dilated [P, scale^2, C, S, S])."""
    NW = g.nwin + scale * scale
    w = windows.reshape(-1, NW, *windows.shape[1:])
    return w[:, :g.nwin].reshape(-1, *windows.shape[1:]), w[:, g.nwin:]


def lowpass(x, L, dtype=torch.float64):
    """L x L^T per plane in `dtype`, returned as float64."""
    L = L.to(dtype)
    return (L @ x.to(dtype) @ L.T).double()


def hires_windows(canvas, L, f, g, scale, dtype=torch.float64):
    """The UNet input [P * NW, C, S, S] of a canvas, float64: the local crops, and the dilated views of canvas + f (L canvas L^T -
    canvas), the plane product taken in `dtype`."""
    x = canvas.double()
    y = x if f == 0.0 else x + f * (lowpass(x, L, dtype) - x)
    loc = po.crop(x, g).reshape(x.shape[0], g.nwin, x.shape[1], g.S, g.S)
    return torch.cat([loc, views(y, scale)], 1).reshape(-1, x.shape[1], g.S, g.S)


def hires_step(canvas, eps, ref, eps_ref, z, wt, L, g, scale, row, dtype=torch.float64):
    """(canvas_out, windows_out) of the fused update: canvas, ref, eps_ref, z [P, C, Hc, Hc], eps NCHW [P * NW, C, S, S].  The two
    window means and the plane product are taken in `dtype`, everything else in float64."""
    p, q, lo, hi, a, b, c, k0, k1, r, gm, f = row
    x = canvas.double()
    loc, dil = split(eps.double(), g, scale)
    x0m = po.fuse(po.x0_windows(canvas, loc, g, row), wt, g, dtype).double()
    em = po.fuse(loc, wt, g, dtype).double()
    if gm != 0.0:
        eg = unviews(dil, scale)
        x0m = (1.0 - gm) * x0m + gm * torch.clamp(p * x + q * eg, lo, hi)
        em = (1.0 - gm) * em + gm * eg
    out = a * x0m + b * em
    if c != 0.0:
        out = out + c * z.double()
    if r != 0.0:
        out = r * (k0 * ref.double() + k1 * eps_ref.double()) + (1.0 - r) * out
    return out, hires_windows(out, L, f, g, scale, dtype)


def upsample(z0, U):
    """ref = U z0 U^T per plane, float64."""
    U = U.double()
    return U @ z0.double() @ U.T


def sample(unet, base, U, L, g, scale, sched, start, eps_ref, draw=None):
    """The float64 sampling loop over a "hires" Schedule: unet(windows fp32 [P * NW, C, S, S], t) -> eps; start = (sqrt(ab_0),
    sqrt(1 - ab_0), f_0) of DDIMScheduler.hires_start; eps_ref the run's canvas-shaped noise; draw() -> the next canvas-shaped
    noise, called where the schedule draws.  Plain count average (wt = 1)."""
    k0, k1, f = start
    ref = upsample(base, U)
    x = (k0 * ref + k1 * eps_ref.double()) * sched.init_noise_sigma
    ones = torch.ones(g.S, g.S, dtype=torch.float64)
    win = hires_windows(x, L, f, g, scale)
    for k, (t, row) in enumerate(zip(sched.timesteps, sched.rows)):
        z = draw().double() if sched.slots(k) else None
        eps = unet(win.float(), t).double()
        x, win = hires_step(x, eps, ref, eps_ref, z, ones, L, g, scale, row)
    return x
