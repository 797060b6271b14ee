"""Float64 restatement of the slot sampler's three kernels on plain tensors (afldm_slot_select / _step / _exchange,
afldm_amd/csrc/slots.hip), and the CPU sampler of ONE request: oracle.unet.unet_forward at the request's timestep, then the row's
update - what a slot must compute whatever its neighbours do.

State per slot b: pos[b] (the row of its last evaluation), end[b]; active in a step iff pos[b] + 1 < end[b].  The functions
below return new tensors and leave their arguments alone."""
import torch

from oracle import unet as ou


def select(row_t, row_temb, pos, end, t_out, temb_table, temb_rows):
    """-> (pos, t_out, active, temb_rows) after the step prologue.  An inactive slot keeps its t_out and its row."""
    pos, t_out, temb_rows = pos.clone(), t_out.clone(), temb_rows.clone()
    active = torch.zeros_like(pos)
    for b in range(pos.numel()):
        if int(pos[b]) + 1 < int(end[b]):
            pos[b] += 1
            p = int(pos[b])
            t_out[b] = row_t[p]
            temb_rows[b] = temb_table[int(row_temb[p])]
            active[b] = 1
    return pos, t_out, active, temb_rows


def ddim_row(x, eps, row):
    """x0 = (x - c1 eps) / c0;  x_out = c2 x0 + c3 eps, in float64."""
    c0, c1, c2, c3 = [float(v) for v in row]
    x, eps = x.double(), eps.double()
    return c2 * ((x - c1 * eps) / c0) + c3 * eps


def step(x, eps_nchw, row_coef, pos, active):
    """-> x after the update (float64): slot b with active[b] takes row_coef[pos[b]], the others are copied."""
    out = x.double().clone()
    for b in range(x.shape[0]):
        if int(active[b]):
            out[b] = ddim_row(x[b], eps_nchw[b], row_coef[int(pos[b])])
    return out


def exchange(cmd, lat, out, fresh, pos, end):
    """-> (lat, out, pos, end) after the boundary: per slot {harvest, refill, begin, end}, the harvest first."""
    lat, out, pos, end = lat.clone(), out.clone(), pos.clone(), end.clone()
    for b in range(lat.shape[0]):
        harvest, refill, begin, stop = [int(v) for v in cmd[b]]
        if harvest >= 0:
            out[harvest] = lat[b]
        if refill >= 0:
            lat[b] = fresh[refill]
            pos[b], end[b] = begin - 1, stop
    return lat, out, pos, end


def sample(sd, cfg, x, schedule):
    """One request [1, C, H, W] through its "ddim" Schedule on the oracle UNet (fp32, CPU), the latents carried in float64."""
    assert schedule.kind == "ddim"
    z = x.double() * schedule.init_noise_sigma
    for t, row in zip(schedule.timesteps, schedule.rows):
        z = ddim_row(z, ou.unet_forward(sd, cfg, z.float(), int(t)), row)
    return z
