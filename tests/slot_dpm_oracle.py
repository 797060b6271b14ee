"""Float64 restatement of afldm_slot_step_kinds (afldm_amd/csrc/slot_kinds.hip) on plain tensors, and the CPU sampler of ONE "dpm"
request: oracle.unet.unet_forward at the request's timestep, then the row's update with the request's own two history planes
- what a slot must compute whatever its neighbours do and whatever its slot held before.

A history plane whose coefficient in the row is exactly 0 does not enter the sum: zeros stand in its place, so NaN left in it
by an earlier occupant reaches no result.  The shift h2 <- h1 moves the plane as it is.  The functions return new tensors and
leave their arguments alone."""
import torch

import slot_oracle as so

KIND_DDIM, KIND_DPM = 0, 1


def dpm_row(x, eps, h1, h2, row):
    """-> (x_out, h1_out, h2_out) in float64:  m0 = p x + q eps;  x_out = a x + b0 m0 + b1 h1 + b2 h2;  h2 <- h1, h1 <- m0."""
    p, q, a, b0, b1, b2 = [float(v) for v in row[:6]]
    x, eps, h1, h2 = x.double(), eps.double(), h1.double(), h2.double()
    m0 = p * x + q * eps
    out = a * x + b0 * m0
    if b1 != 0.0:
        out = out + b1 * h1
    if b2 != 0.0:
        out = out + b2 * h2
    return out, m0, h1.clone()


def step_kinds(x, eps_nchw, hist, row_coef, row_kind, pos, active):
    """-> (x, hist) after the update (float64): slot b with active[b], pos[b] inside the table and a known kind takes
    row_coef[pos[b]] as its kind says; every other slot, and a "ddim" slot's history, is copied."""
    out, h = x.double().clone(), hist.double().clone()
    R = row_coef.shape[0]
    for b in range(x.shape[0]):
        r = int(pos[b])
        if not int(active[b]) or not 0 <= r < R:
            continue
        if int(row_kind[r]) == KIND_DDIM:
            out[b] = so.ddim_row(x[b], eps_nchw[b], row_coef[r][:4])
        elif int(row_kind[r]) == KIND_DPM:
            out[b], h[0, b], h[1, b] = dpm_row(x[b], eps_nchw[b], hist[0, b], hist[1, b], row_coef[r])
    return out, h


def sample_with(eps_fn, x, schedule):
    """One request through its "dpm" Schedule with eps_fn(z, t) as the model, the latents and the history in float64; the
    history starts as NaN: a fresh request reads none of it."""
    assert schedule.kind == "dpm"
    z = x.double() * schedule.init_noise_sigma
    h1 = torch.full_like(z, float("nan"))
    h2 = torch.full_like(z, float("nan"))
    for t, row in zip(schedule.timesteps, schedule.rows):
        z, h1, h2 = dpm_row(z, eps_fn(z, int(t)), h1, h2, row)
    return z


def sample(sd, cfg, x, schedule):
    """One request [1, C, H, W] through its "dpm" Schedule on the oracle UNet (fp32, CPU), as slot_oracle.sample for "ddim"."""
    from oracle import unet as ou
    return sample_with(lambda z, t: ou.unet_forward(sd, cfg, z.float(), t), x, schedule)
