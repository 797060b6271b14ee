"""MultiDiffusion's window arithmetic restated in torch on the CPU, float64 unless told otherwise: the yardstick of
csrc/pano.hip (afldm_pano_step, afldm_window_fuse, afldm_window_crop) and of MyLDMPipeline.panorama_latents.  Not a test module.

A geometry is anything with Hc, Wc, S, oy, ox, wrap_y, wrap_x (afldm_amd.panorama.Geometry).  Window k = iy * nx + ix of canvas P
is batch entry P * nwin + k and covers rows (oy[iy] + u) mod Hc, columns (ox[ix] + v) mod Wc.  Sums over the covering windows run
in ascending k, as the kernels' do, so that `dtype=torch.float32` is the same sum in fp32 (the second term of the tests' bound)."""
import torch


def indices(g):
    """[(rows, cols)] per window in k order: LongTensors of the S canvas rows / columns the window covers."""
    ar = torch.arange(g.S)
    out = []
    for oy in g.oy:
        for ox in g.ox:
            ys, xs = oy + ar, ox + ar
            assert (g.wrap_y or int(ys[-1]) < g.Hc) and (g.wrap_x or int(xs[-1]) < g.Wc), "a window leaves a non-wrapping axis"
            out.append((ys % g.Hc, xs % g.Wc))
    return out


def crop(canvas, g):
    """[P, C, Hc, Wc] -> [P * nwin, C, S, S], exact in any dtype."""
    wins = [canvas[:, :, ys[:, None], xs[None, :]] for ys, xs in indices(g)]          # nwin x [P, C, S, S]
    return torch.stack(wins, 1).reshape(-1, canvas.shape[1], g.S, g.S)


def fuse(windows, wt, g, dtype=torch.float64):
    """[P * nwin, C, S, S] -> [P, C, Hc, Wc]: sum_k wt win_k / sum_k wt over the covering windows, ascending k, in `dtype`."""
    idx = indices(g)
    n = len(idx)
    w = windows.to(dtype).reshape(-1, n, windows.shape[1], g.S, g.S)
    wt = wt.to(dtype)
    A = torch.zeros(w.shape[0], w.shape[2], g.Hc, g.Wc, dtype=dtype)
    W = torch.zeros(g.Hc, g.Wc, dtype=dtype)
    for k, (ys, xs) in enumerate(idx):
        A[:, :, ys[:, None], xs[None, :]] += wt * w[:, k]
        W[ys[:, None], xs[None, :]] += wt
    assert bool((W > 0).all()), "an element no window covers"
    return A / W


def x0_windows(canvas, eps, g, row):
    """Every window's clean-latent prediction clamp(p x + q e_k, lo, hi), float64: [P * nwin, C, S, S]; eps NCHW likewise."""
    p, q, lo, hi = row[:4]
    return torch.clamp(p * crop(canvas.double(), g) + q * eps.double(), lo, hi)


def pano_step(canvas, eps, z, wt, g, row, dtype=torch.float64):
    """(canvas_out, windows_out) of the fused update on the "sde" row (p, q, lo, hi, a, b, d, c): canvas [P, C, Hc, Wc], eps NCHW
    [P * nwin, C, S, S], z the canvas-shaped noise (not looked at where c == 0).  The means are taken in `dtype`."""
    a, b, d, c = row[4:8]
    x = canvas.double()
    out = a * x + b * fuse(x0_windows(canvas, eps, g, row), wt, g, dtype).double() + d * fuse(eps.double(), wt, g, dtype).double()
    if c != 0.0:
        out = out + c * z.double()
    return out, crop(out, g)


def sde_single(x, eps, z, row):
    """The plain stochastic update, float64: what pano_step must reduce to with one window."""
    p, q, lo, hi, a, b, d, c = row
    x, eps = x.double(), eps.double()
    out = a * x + b * torch.clamp(p * x + q * eps, lo, hi) + d * eps
    return out + c * z.double() if c != 0.0 else out


def sample(unet, canvas, g, sched, draw=None):
    """The float64 sampling loop over a "pano" Schedule: unet(windows fp32 [P * nwin, C, S, S], t) -> eps; draw() -> the next
    canvas-shaped noise, called where the schedule draws.  Plain count average (wt = 1)."""
    x = canvas.double() * sched.init_noise_sigma
    ones = torch.ones(g.S, g.S, dtype=torch.float64)
    for k, (t, row) in enumerate(zip(sched.timesteps, sched.rows)):
        z = draw().double() if sched.slots(k) else None
        eps = unet(crop(x, g).float(), t).double()
        x, _ = pano_step(x, eps, z, ones, g, row)
    return x
