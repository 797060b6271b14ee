"""numpy restatement of the counter-based noise stream and the "seeded" update (include/afldm_hip_noise.h,
afldm_amd/csrc/philox.hpp, afldm_amd/csrc/noise.hip), and the CPU sampler of ONE seeded request.

  philox(counters, key)            Philox-4x32-10 as in Random123, on uint32 arrays
  words(seed, groups, ...)         the words of the counters (g0 + g, ordinal, slot, c3) under the seed's key
  normals(seed, ordinal, n, ...)   the first n normals of a sample's stream, float64 (dtype=np.float32: the same formula evaluated
                                   in float32 - what the formats themselves lose, the yardstick of the device's accuracy)
  update32(x, e, z, row)           the update in float32 in the stated order: every product rounded, sums left to right
  update64(x, e, z, row)           the same formula in float64
  sample(sd, cfg, start, schedule, seed)   one request through its "seeded" Schedule on the oracle UNet, as slot_oracle.sample"""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(counters, key):
    """counters: uint32 [..., 4]; key: (k0, k1) -> uint32 [..., 4].  One round:
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped after the round."""
    c = [np.asarray(counters)[..., j].astype(np.uint64) for j in range(4)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def key_of(seed):
    seed = int(seed)
    assert 0 <= seed < 2 ** 63
    return seed & MASK, seed >> 32


def words(seed, groups, g0=0, ordinal=0, slot=0, c3=0):
    """uint32 [groups, 4]: the words of the counters (g0 + g, ordinal, slot, c3), each taken modulo 2^32."""
    c = np.zeros((int(groups), 4), dtype=np.uint32)
    c[:, 0] = ((int(g0) + np.arange(int(groups), dtype=np.uint64)) & np.uint64(MASK)).astype(np.uint32)
    c[:, 1], c[:, 2], c[:, 3] = int(ordinal) & MASK, int(slot) & MASK, int(c3) & MASK
    return philox(c, key_of(seed))


def normals(seed, ordinal, n, slot=0, dtype=np.float64):
    """The first n values of the stream of (seed, ordinal, slot): u = ((r >> 9) + 0.5) 2^-23 (exact in either dtype), then
    (z0, z1) = sqrt(-2 ln u0) (cos 2 pi u1, sin 2 pi u1) and (z2, z3) likewise from (u2, u3), all in `dtype`."""
    r = words(seed, (int(n) + 3) // 4, 0, ordinal, slot)
    u = ((r >> np.uint32(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23)
    rad = np.sqrt(dtype(-2.0) * np.log(u[:, 0::2]))
    ang = dtype(2.0 * np.pi) * u[:, 1::2]
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1)          # [groups, 2 pairs, (cos, sin)]
    assert z.dtype == dtype
    return z.reshape(-1)[:int(n)]


def noise(seeds, ordinals, shape, slot=0, dtype=np.float64):
    """[B, C, H, W]: sample b's stream at ordinals[b], in its own flat [C, H, W] order."""
    B, n = shape[0], int(np.prod(shape[1:]))
    return np.stack([normals(seeds[b], ordinals[b], n, slot, dtype) for b in range(B)]).reshape(shape)


def _clamp_nan(t, lo, hi):
    return np.where(t < lo, lo, np.where(t > hi, hi, t))


def update32(x, e, z, row):
    """t = rn(p x) + rn(q e);  x0 = clamp_nan(t, lo, hi);  out = ((rn(a x) + rn(b x0)) + rn(d e)) + rn(c z), every operation a float32
    numpy ufunc of its own (no fused multiply-add).  row: the eight floats, rounded to float32 as Schedule.table rounds them."""
    f = np.float32
    p, q, lo, hi, a, b, d, c = [f(v) for v in np.asarray(row, dtype=np.float64).astype(np.float32)]
    x, e, z = np.asarray(x, dtype=f), np.asarray(e, dtype=f), np.asarray(z, dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p * x + q * e
        x0 = _clamp_nan(t, lo, hi).astype(f)
        out = ((a * x + b * x0) + d * e) + c * z
    assert out.dtype == f
    return out


def update64(x, e, z, row):
    p, q, lo, hi, a, b, d, c = [float(v) for v in row]
    x0 = torch.clamp(p * x + q * e, lo, hi)
    return a * x + b * x0 + d * e + c * z


def sample(sd, cfg, start, schedule, seed):
    """One request [1, C, H, W] through its "seeded" Schedule on the oracle UNet (fp32, CPU), the latents carried in float64;
    the noise of step k is normals(seed, k), zeros where the row's c is 0."""
    from oracle import unet as ou
    assert schedule.kind == "seeded"
    z = start.double() * schedule.init_noise_sigma
    for k, (t, row) in enumerate(zip(schedule.timesteps, schedule.rows)):
        n = torch.from_numpy(normals(seed, k, z.numel())).reshape(z.shape) if row[7] != 0.0 else torch.zeros_like(z)
        z = update64(z, ou.unet_forward(sd, cfg, z.float(), int(t)).double(), n, row)
    return z
