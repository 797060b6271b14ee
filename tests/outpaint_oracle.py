"""Outpainting (RePaint on a MultiDiffusion canvas) restated in torch on the CPU, float64 unless told otherwise, on top of
tests/pano_oracle.py (crop, fuse, x0_windows): the yardstick of afldm_pano_repaint_step and of MyLDMPipeline.outpaint_latents.
Not a test module.

The row is "repaint"'s, (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0); zs = (z_k, z_u, z_b), canvas-shaped, an entry not looked at
(it may be None) where its coefficient - k1, c, u1 - is 0.  Where the mask is exactly 1 the model's side is left out of the blend
(as the kernel leaves it out), so that a kept element is a function of the known content and the noise alone."""
import torch

import pano_oracle as po


def outpaint_step(canvas, eps, known, mask, zs, wt, g, row, dtype=torch.float64):
    """(canvas_out, windows_out, unknown, knownp): canvas, known [P, C, Hc, Wc], mask [P | 1, 1, Hc, Wc], eps NCHW
    [P * nwin, C, S, S].  The two means over the covering windows are taken in `dtype`, everything else in float64."""
    p, q, lo, hi, a, b, c, k0, k1, u0, u1 = row[:11]
    zk, zu, zb = zs
    unknown = a * po.fuse(po.x0_windows(canvas, eps, g, row), wt, g, dtype).double() + b * po.fuse(eps.double(), wt, g, dtype).double()
    if c != 0.0:
        unknown = unknown + c * zu.double()
    knownp = k0 * known.double()
    if k1 != 0.0:
        knownp = knownp + k1 * zk.double()
    m = mask.double().expand(canvas.shape[0], 1, g.Hc, g.Wc)
    y = torch.where(m == 1.0, m * knownp, m * knownp + (1.0 - m) * unknown)
    out = u0 * y
    if u1 != 0.0:
        out = out + u1 * zb.double()
    return out, po.crop(out, g), unknown, knownp


def repaint_single(x, eps, known, mask, zs, row):
    """The plain RePaint update (csrc/repaint.hip), float64: what outpaint_step must reduce to with one window of weight 1."""
    p, q, lo, hi, a, b, c, k0, k1, u0, u1 = row[:11]
    zk, zu, zb = [None if z is None else z.double() for z in zs]
    x, eps, m = x.double(), eps.double(), mask.double()
    x0 = torch.clamp(p * x + q * eps, lo, hi)
    unknown = a * x0 + b * eps + (c * zu if c != 0.0 else 0.0)
    knownp = k0 * known.double() + (k1 * zk if k1 != 0.0 else 0.0)
    y = m * knownp + (1.0 - m) * unknown
    return u0 * y + (u1 * zb if u1 != 0.0 else 0.0)


def sample(unet, canvas, known, mask, g, sched, draw=None):
    """The float64 sampling loop over an "outpaint" Schedule: unet(windows fp32 [P * nwin, C, S, S], t) -> eps; draw() -> the next
    canvas-shaped noise, called once per slot the schedule draws, in step and slot order.  Plain count average (wt = 1)."""
    x = canvas.double() * sched.init_noise_sigma
    ones = torch.ones(g.S, g.S, dtype=torch.float64)
    for k, (t, row) in enumerate(zip(sched.timesteps, sched.rows)):
        on = sched.slots(k)
        zs = [draw().double() if j in on else None for j in range(3)]
        eps = unet(po.crop(x, g).float(), t).double()
        x = outpaint_step(x, eps, known, mask, zs, ones, g, row)[0]
    return x
