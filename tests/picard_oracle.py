"""Float64 restatement of parallel-in-time sampling (afldm_amd/csrc/picard.hip, PicardEngine): Picard sweeps over a window of
`window` consecutive rows of one "ddim" Schedule.  Per image: states X[0 .. W], estimates of x_base .. x_{base + W}, X[0] exact.

  1. evaluate  e_j = eps(X[j], t_{base + j}), j = 0 .. W - 1 (a row with base + j >= n is inactive: not used)
  2. sweep     Y[0] = X[0];  Y[j + 1] = U_{base + j}(Y[j], e_j) for an active j, Y[j] for an inactive one;
               err_j = mean (Y[j] - X[j])^2, j = 1 .. W, 0 for a row made by an inactive j - 1
  3. stride    s = min({j in 1 .. W : err_j > tol^2} U {W});  s = min(s, n - base);  a finished image (base == n): s = 0
  4. slide     X[j] = Y[min(j + s, W)];  base += s

`decide` and `slide` are the integer logic on plain values (what tests/test_gpu_picard.py holds the kernels against); `sample`
is the sampler over slot_oracle.ddim_row and an eps function evaluated one row at a time with that row's own timestep."""
import torch

import slot_oracle as so


def decide(errs, base, n, window, tol2):
    """The stride of one image: errs[j - 1] = err_j, j = 1 .. window."""
    if base >= n:
        return 0
    s = window
    for j in range(1, window + 1):
        if base + j - 1 < n and errs[j - 1] > tol2:
            s = j
            break
    return min(s, n - base)


def sweep(X, eps, rows, base):
    """X [W + 1, ...], eps [W, ...] of ONE image -> (Y [W + 1, ...] float64, [err_1 .. err_W])."""
    W, n = X.shape[0] - 1, len(rows)
    Y, errs = [X[0].double()], []
    for j in range(W):
        if base + j < n:
            Y.append(so.ddim_row(Y[j], eps[j], rows[base + j]))
            errs.append(float((Y[j + 1] - X[j + 1].double()).pow(2).mean()))
        else:
            Y.append(Y[j])
            errs.append(0.0)
    return torch.stack(Y), errs


def slide(Y, s):
    """X after the slide by s >= 1."""
    W = Y.shape[0] - 1
    return torch.stack([Y[min(j + s, W)] for j in range(W + 1)])


def sample(eps_fn, x, schedule, window, tolerance):
    """x [P, C, H, W] -> (latents float64 [P, C, H, W], strides [iteration][image], errs [iteration][image][W]).  eps_fn(z, r): the
    model's output (float64 or fp32) for ONE state z [1, C, H, W] at row r of the schedule (timestep schedule.timesteps[r])."""
    assert schedule.kind == "ddim" and window >= 1
    n, P, rows = len(schedule.rows), x.shape[0], schedule.rows
    X = [torch.stack([x[p].double() * schedule.init_noise_sigma] * (window + 1)) for p in range(P)]
    base, strides, errs = [0] * P, [], []
    while min(base) < n:
        assert len(strides) < n, "more than n iterations"
        took, seen = [], []
        for p in range(P):
            if base[p] >= n:
                took.append(0)
                seen.append([0.0] * window)
                continue
            eps = torch.stack([eps_fn(X[p][j][None], base[p] + j)[0].double() if base[p] + j < n else torch.zeros_like(X[p][j])
                               for j in range(window)])
            Y, e = sweep(X[p], eps, rows, base[p])
            s = decide(e, base[p], n, window, tolerance ** 2)
            X[p] = slide(Y, s)
            base[p] += s
            took.append(s)
            seen.append(e)
        strides.append(took)
        errs.append(seen)
    return torch.stack([X[p][0] for p in range(P)]), strides, errs


def row_only_iterations(n, window):
    """Iterations at tolerance 0 when eps depends on the row only.  ONE sweep then computes the exact chain, but the decision
    only sees which estimates the sweep confirmed.  A fresh window (every estimate a copy of X[0]) confirms nothing: s = 1, and
    the slide leaves window - 1 exact estimates and one stale copy; the next sweep confirms those and computes one more: s =
    window, and the slide by a whole window leaves a fresh window again.  So the strides go 1, W, 1, W, ... until the rows run
    out: two iterations per W + 1 rows.  Up to n = W + 1 rows, and for W = 1, this is 1 + ceil((n - 1) / W)."""
    return 2 * (n // (window + 1)) + min(n % (window + 1), 2)


def unet_eps(sd, cfg, schedule):
    """eps_fn of the oracle UNet (fp32, CPU), as slot_oracle.sample evaluates it."""
    from oracle import unet as ou
    return lambda z, r: ou.unet_forward(sd, cfg, z.float(), int(schedule.timesteps[r]))
