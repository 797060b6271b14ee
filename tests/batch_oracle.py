"""Batch-position relations (importable on the CPU): checks that need no reference and no tolerance.

Every operator of the UNet works on one sample at a time, so for ANY batched function f of it
    rotation:  f(roll(x, r, 0)) == roll(f(x), r, 0)                      bit for bit, and
    poison:    overwriting sample p leaves every other sample's output    bit for bit
whatever tile, workgroup or split a sample lands in.  A kernel that packs several samples into one tile, walks (sample, block)
items persistently or switches its plan on the batch can break either: a neighbour's GroupNorm statistics, time-embedding row
or halo row, an index that is right only for some slots.  With i.i.d. samples such a fault is a percent of 1/B of the tensor
and passes any rel-RMS bound; distinct_batch() gives every sample its own scale and offset, and the relations are exact.

A function may take several batched tensors (x, time embedding, residual: a tuple, all rolled / poisoned together) and return a
tensor or a tuple of tensors whose dim 0 is the batch; GroupNorm partial sums riding on an output as `.gn_partial`
[B, S, C, 2] count as one more output.
"""
import math

import torch

BIG = "big"            # check_poison value: the sample's own data times 1e4 (finite)


def distinct_batch(B, shape, seed, dtype=torch.float32):
    """[B, *shape] on the CPU in `dtype`: sample b is Gaussian with scale 0.5 + 1.5 b / B and offset (-1)^b (0.25 + 0.75 b / B) -
    neighbours differ in mean, variance and sign of the mean."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B,) + tuple(shape), generator=g)
    b = torch.arange(B, dtype=torch.float32).view((B,) + (1,) * len(shape))
    scale = 0.5 + 1.5 * b / B
    offset = torch.where(b.long() % 2 == 0, 1.0, -1.0) * (0.25 + 0.75 * b / B)
    return (x * scale + offset).to(dtype)


def _tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def outputs(y):
    """The batched tensors of a result: every tensor of the tuple, each followed by its `.gn_partial` if it carries one."""
    out = []
    for t in _tuple(y):
        out.append(t)
        st = getattr(t, "gn_partial", None)
        if st is not None:
            out.append(st)
    return out


def run(f, x):
    return outputs(f(*_tuple(x)))


def _describe(got, want):
    """Which batch positions differ, and by how much at most."""
    g, w = got.detach().double().flatten(1).cpu(), want.detach().double().flatten(1).cpu()
    bad = ((g != w) & ~(torch.isnan(g) & torch.isnan(w))).any(1) | (torch.isnan(g) != torch.isnan(w)).any(1)
    pos = bad.nonzero().flatten().tolist()
    d = (g - w).abs()
    d = d[torch.isfinite(d)]
    top = float(d.max()) if d.numel() else math.nan
    scale = float(w[torch.isfinite(w)].abs().max()) if torch.isfinite(w).any() else math.nan
    return pos, top, scale


def check_rotation(f, x, r, base=None, what=""):
    """assert torch.equal(f(roll(x, r, 0)), roll(f(x), r, 0)) for every output.  base: run(f, x) from an earlier call (saves
    the clean run); returned for the next one."""
    xs = _tuple(x)
    B = xs[0].shape[0]
    if base is None:
        base = run(f, xs)
    got = run(f, tuple(torch.roll(t, r, 0).contiguous() for t in xs))
    assert len(got) == len(base), f"{what}: {len(got)} outputs after the rotation, {len(base)} before"
    for i, (g, b) in enumerate(zip(got, base)):
        want = torch.roll(b, r, 0)
        assert g.shape == want.shape and g.shape[0] == B, f"{what}: output {i} has shape {tuple(g.shape)}, batch {B}"
        if not torch.equal(g, want):
            pos, top, scale = _describe(g, want)
            src = [(p - r) % B for p in pos]
            raise AssertionError(f"{what}: rotation by {r} of batch {B}, output {i}: {len(pos)} positions differ - rotated "
                                 f"positions {pos[:24]} (samples {src[:24]} of the unrotated batch), largest difference {top:.4g} "
                                 f"(max |value| {scale:.4g})")
    return base


def poisoned(x, p, value):
    """Copies of the batched tensors with samples `p` (an index or several) overwritten: value NaN (or any float) fills the
    sample, BIG multiplies its own data by 1e4.  Integer tensors are left alone."""
    ps = _tuple(p)
    out = []
    for t in _tuple(x):
        t = t.clone()
        if t.is_floating_point():
            for q in ps:
                if isinstance(value, str):
                    assert value == BIG
                    t[q] = t[q] * 1e4
                else:
                    t[q] = value
        out.append(t)
    return tuple(out)


def check_poison(f, x, p, value=math.nan, base=None, what=""):
    """Sample(s) p overwritten (see poisoned): every OTHER sample's output must be bit-identical to the clean run, in every
    output; with a NaN, the first output of every poisoned sample must hold a non-finite value."""
    xs = _tuple(x)
    B = xs[0].shape[0]
    ps = _tuple(p)
    assert all(0 <= q < B for q in ps), (ps, B)
    if base is None:
        base = run(f, xs)
    got = run(f, poisoned(xs, ps, value))
    keep = torch.ones(B, dtype=torch.bool)
    keep[list(ps)] = False
    assert len(got) == len(base), f"{what}: {len(got)} outputs with the poison, {len(base)} without"
    for i, (g, b) in enumerate(zip(got, base)):
        assert g.shape == b.shape and g.shape[0] == B, f"{what}: output {i} has shape {tuple(g.shape)}, batch {B}"
        k = keep.to(g.device)
        if not torch.equal(g[k], b[k]):
            pos, top, scale = _describe(g[k], b[k])
            idx = keep.nonzero().flatten()[pos].tolist()
            raise AssertionError(f"{what}: sample(s) {list(ps)} of batch {B} poisoned with {value}, output {i}: samples {idx[:24]} "
                                 f"changed ({len(idx)} in all), largest finite difference {top:.4g} (max |value| {scale:.4g})")
    if not isinstance(value, str) and math.isnan(value):
        for q in ps:
            assert not bool(torch.isfinite(got[0][q]).all()), f"{what}: sample {q} was all NaN and its output is finite: it was not read"
    return base
