"""numpy restatement of the image-conditioned slot updates (include/afldm_hip_edit.h, afldm_amd/csrc/edit.hip) and the CPU
samplers of ONE "seeded_sdedit" / "seeded_repaint" request, on the noise stream of tests/noise_oracle.py.

  NOISE_SLOTS                           which stream slot each noise of a kind is, and at which ordinal
  sdedit32(x, e, o, m, z, zu, row)      kind 3 in float32 in the stated order: every product rounded, sums left to right
  repaint32(x, e, kn, m, zk, zu, zb, row)   kind 4 likewise
  sdedit64 / repaint64                  the same formulas in float64 (torch)
  slot_step(...)                        afldm_slot_step_edit's kinds 3 and 4 over a batch of slots, the noises given by a callable
  sample_sdedit / sample_repaint        one request through its Schedule on the oracle UNet, float64 latents, noise_oracle.normals"""
import numpy as np
import torch

import noise_oracle as no

KIND_SDEDIT, KIND_REPAINT = 3, 4
# noise name -> (stream slot, whether it sits at the row's ordinal - otherwise at ordinal 0), and the row field of its coefficient
NOISE_SLOTS = {KIND_SDEDIT: {"zu": (0, True, 6), "z": (1, False, 8)},
               KIND_REPAINT: {"zk": (0, True, 8), "zu": (1, True, 6), "zb": (2, True, 10)}}


def _row32(row, n):
    return [np.float32(v) for v in np.asarray(row, dtype=np.float64).astype(np.float32)[:n]]


def _f32(*arrays):
    return [np.asarray(a, dtype=np.float32) for a in arrays]


def sdedit32(x, e, o, m, z, zu, row):
    """t = rn(p x) + rn(q e);  x0 = clamp_nan(t, lo, hi);  xp = (rn(a x0) + rn(b e)) + rn(c z_u);  held = rn(k0 o) + rn(k1 z);
    out = (m <= thr) ? held : xp - every operation a float32 numpy ufunc of its own."""
    p, q, lo, hi, a, b, c, k0, k1, thr = _row32(row, 10)
    x, e, o, m, z, zu = _f32(x, e, o, m, z, zu)
    with np.errstate(invalid="ignore", over="ignore"):
        px, qe = p * x, q * e
        t = px + qe
        x0 = no._clamp_nan(t, lo, hi).astype(np.float32)
        ax0, be, cz = a * x0, b * e, c * zu
        xp = (ax0 + be) + cz
        k0o, k1z = k0 * o, k1 * z
        held = k0o + k1z
        out = np.where(m <= thr, held, xp)
    assert out.dtype == np.float32
    return out


def repaint32(x, e, kn, m, zk, zu, zb, row):
    """x0 as sdedit32;  unknown = (rn(a x0) + rn(b e)) + rn(c z_u);  knownp = rn(k0 kn) + rn(k1 z_k);
    y = rn(m knownp) + rn(rn(1 - m) unknown);  out = rn(u0 y) + rn(u1 z_b)."""
    p, q, lo, hi, a, b, c, k0, k1, u0, u1 = _row32(row, 11)
    x, e, kn, m, zk, zu, zb = _f32(x, e, kn, m, zk, zu, zb)
    with np.errstate(invalid="ignore", over="ignore"):
        px, qe = p * x, q * e
        t = px + qe
        x0 = no._clamp_nan(t, lo, hi).astype(np.float32)
        ax0, be, cz = a * x0, b * e, c * zu
        unknown = (ax0 + be) + cz
        k0k, k1z = k0 * kn, k1 * zk
        knownp = k0k + k1z
        om = np.float32(1.0) - m
        mk, ou = m * knownp, om * unknown
        y = mk + ou
        u0y, u1z = u0 * y, u1 * zb
        out = u0y + u1z
    assert out.dtype == np.float32
    return out


def sdedit64(x, e, o, m, z, zu, row):
    p, q, lo, hi, a, b, c, k0, k1, thr = [float(v) for v in row[:10]]
    x0 = torch.clamp(p * x + q * e, lo, hi)
    return torch.where(m <= thr, k0 * o + k1 * z, a * x0 + b * e + c * zu)


def repaint64(x, e, kn, m, zk, zu, zb, row):
    p, q, lo, hi, a, b, c, k0, k1, u0, u1 = [float(v) for v in row[:11]]
    x0 = torch.clamp(p * x + q * e, lo, hi)
    y = m * (k0 * kn + k1 * zk) + (1 - m) * (a * x0 + b * e + c * zu)
    return u0 * y + u1 * zb


def slot_step(x, e, cond, cmask, row_coef, row_kind, row_ord, pos, active, seeds, noise):
    """afldm_slot_step_edit's kinds 3 and 4 on the host.  x, e (eps as NCHW), cond: float32 [B, C, H, W] arrays; cmask [B, 1, H, W];
    row_coef [R, 12]; noise(seed, ordinal, slot) -> float32 [C, H, W], asked for only where the coefficient is not 0.  Returns
    the new x; a slot that is inactive, out of range or of another kind keeps its x."""
    out = np.array(x, dtype=np.float32, copy=True)
    R = len(row_kind)
    for b in range(out.shape[0]):
        s = int(pos[b])
        if not int(active[b]) or not 0 <= s < R or int(row_kind[s]) not in NOISE_SLOTS:
            continue
        kind, row = int(row_kind[s]), np.asarray(row_coef[s], dtype=np.float64)
        zs = {}
        for name, (slot, at_row, field) in NOISE_SLOTS[kind].items():
            on = np.float32(row[field]) != 0
            zs[name] = noise(int(seeds[b]), int(row_ord[s]) if at_row else 0, slot) if on else np.zeros(out.shape[1:], np.float32)
        m = np.broadcast_to(cmask[b], out.shape[1:])
        if kind == KIND_SDEDIT:
            out[b] = sdedit32(x[b], e[b], cond[b], m, zs["z"], zs["zu"], row)
        else:
            out[b] = repaint32(x[b], e[b], cond[b], m, zs["zk"], zs["zu"], zs["zb"], row)
    return out


def _normal(seed, ordinal, slot, like, on):
    if not on:
        return torch.zeros_like(like)
    return torch.from_numpy(no.normals(seed, ordinal, like.numel(), slot)).reshape(like.shape)


def sdedit_start(orig, k0s, k1s, seed):
    """k0_start orig + k1_start z in float64, z the stream's slot 1 at ordinal 0."""
    orig = orig.double()
    return k0s * orig + k1s * _normal(seed, 0, 1, orig, True)


def sample_sdedit(sd, cfg, orig, cmap, schedule, start, seed):
    """One request [1, C, H, W] through its "seeded_sdedit" Schedule on the oracle UNet (fp32, CPU), the latents carried in float64
    from `start` (sdedit_start); z_u of step k is normals(seed, k, slot 0), the fixed z normals(seed, 0, slot 1)."""
    from oracle import unet as ou
    assert schedule.kind == "seeded_sdedit"
    x, o, m = start.double(), orig.double(), cmap.double().expand_as(orig)
    z = _normal(seed, 0, 1, x, True)
    for k, (t, row) in enumerate(zip(schedule.timesteps, schedule.rows)):
        e = ou.unet_forward(sd, cfg, x.float(), int(t)).double()
        x = sdedit64(x, e, o, m, z if row[8] != 0.0 else torch.zeros_like(x), _normal(seed, k, 0, x, row[6] != 0.0), row)
    return x


def sample_repaint(sd, cfg, start, known, mask, schedule, seed):
    """One request through its "seeded_repaint" Schedule likewise: z_k, z_u, z_b of step k are normals(seed, k, slot 0 / 1 / 2)."""
    from oracle import unet as ou
    assert schedule.kind == "seeded_repaint"
    x, kn, m = start.double() * schedule.init_noise_sigma, known.double(), mask.double().expand_as(known)
    for k, (t, row) in enumerate(zip(schedule.timesteps, schedule.rows)):
        e = ou.unet_forward(sd, cfg, x.float(), int(t)).double()
        x = repaint64(x, e, kn, m, _normal(seed, k, 0, x, row[8] != 0.0), _normal(seed, k, 1, x, row[6] != 0.0),
                      _normal(seed, k, 2, x, row[10] != 0.0), row)
    return x
