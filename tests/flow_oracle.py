"""CPU oracle of the forward bilinear splat (afldm_flow_splat), written from its specification, vectorised in NumPy.

Source (i, j) lands at ci = i + s * flow[0, i, j], cj = j + s * flow[1, i, j]: fp32, the product rounded before the add.
i1 = int(ci) truncated towards zero, i2 = i1 + 1 (same for j); each of the four targets inside the plane receives
coef = (1 - |ci - gi|) * (1 - |cj - gj|) (every operation in fp32; negative for some targets when ci or cj < 0):
res[:, gi, gj] += x[:, i, j] * coef (the product in fp32), cnt[gi, gj] += coef.  Only the SUMS are float64 here, so the
distance of any fp32 summation order from this oracle is bounded per target by (k + 1) * 2^-23 * mag, with k the number of
contributions with a non-zero coefficient (integer landing points hand their second neighbours an exact 0, which no order
of summation can turn into an error) and mag the sum of their magnitudes."""
import numpy as np

EPS = 2.0 ** -23


def splat(x, flow, s=1.0):
    """x [C, H, W], flow [2, H, W], s scalar -> dict of res [C, H, W] f64, cnt [H, W] f64, k [H, W] int, mag [C, H, W] f64
    (sum |coef * x|), cmag [H, W] f64 (sum |coef|), occ [H, W] bool (cnt > 0 is false), ambiguous [H, W] bool."""
    x = np.asarray(x, dtype=np.float32)
    flow = np.asarray(flow, dtype=np.float32)
    C, H, W = x.shape
    s = np.float32(s)
    ii, jj = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ci = (ii + (s * flow[0]).astype(np.float32)).astype(np.float32)
    cj = (jj + (s * flow[1]).astype(np.float32)).astype(np.float32)
    ok = np.isfinite(ci) & np.isfinite(cj) & (np.abs(ci) < 2 ** 30) & (np.abs(cj) < 2 ** 30)
    i1 = np.trunc(np.where(ok, ci, -10)).astype(np.int64)
    j1 = np.trunc(np.where(ok, cj, -10)).astype(np.int64)
    res, mag = np.zeros((C, H * W)), np.zeros((C, H * W))
    cnt, cmag, k = np.zeros(H * W), np.zeros(H * W), np.zeros(H * W, dtype=np.int64)
    one = np.float32(1)
    for di in (0, 1):
        for dj in (0, 1):
            gi, gj = i1 + di, j1 + dj
            inb = ok & (gi >= 0) & (gi < H) & (gj >= 0) & (gj < W)
            coef = ((one - np.abs(ci - gi.astype(np.float32))) * (one - np.abs(cj - gj.astype(np.float32)))).astype(np.float32)
            idx = (gi * W + gj)[inb]
            c = coef[inb]
            cnt += np.bincount(idx, weights=c.astype(np.float64), minlength=H * W)
            cmag += np.bincount(idx, weights=np.abs(c).astype(np.float64), minlength=H * W)
            k += np.bincount(idx[c != 0], minlength=H * W)          # a zero coefficient adds exactly nothing, in any order
            for ch in range(C):
                v = (x[ch][inb] * c).astype(np.float32).astype(np.float64)
                res[ch] += np.bincount(idx, weights=v, minlength=H * W)
                mag[ch] += np.bincount(idx, weights=np.abs(v), minlength=H * W)
    out = dict(res=res.reshape(C, H, W), cnt=cnt.reshape(H, W), k=k.reshape(H, W), mag=mag.reshape(C, H, W),
               cmag=cmag.reshape(H, W))
    out["occ"] = ~(out["cnt"] > 0)
    out["bound"] = (out["k"] + 1) * EPS * out["mag"]
    out["ambiguous"] = (out["k"] > 0) & (np.abs(out["cnt"]) <= (out["k"] + 1) * EPS * out["cmag"])
    return out


def pick(o, ds, fill=None):
    """The oracle at every ds-th pixel: (res, bound, occ, ambiguous); fill [C, H, W] (full resolution) replaces res where occ."""
    res, occ = o["res"][:, ::ds, ::ds], o["occ"][::ds, ::ds]
    bound = o["bound"][:, ::ds, ::ds]
    if fill is not None:
        f = np.asarray(fill, dtype=np.float64)[:, ::ds, ::ds]
        res = np.where(occ[None], f, res)
        bound = np.where(occ[None], 0.0, bound)
    return res, bound, occ, o["ambiguous"][::ds, ::ds]


def pool(o, ds, fill=None):
    """collect_noise_pixel on the oracle: sum over ds x ds blocks of (fill * occ + res * (1 - occ)) / ds, and its bound: the
    per-target bounds of the kept terms add up, and the fp32 sum of the ds^2 terms of a block in any order, plus the
    division, errs by at most (ds^2 + 1) * 2^-23 * sum |term| (the same rule with k = ds^2)."""
    C, H, W = o["res"].shape
    occ = o["occ"][None]
    f = np.zeros_like(o["res"]) if fill is None else np.asarray(fill, dtype=np.float64)
    v = np.where(occ, f, o["res"])
    b = np.where(occ, 0.0, o["bound"])
    blk = lambda a: a.reshape(C, H // ds, ds, W // ds, ds).sum(axis=(2, 4))
    return blk(v) / ds, (blk(b) + (ds * ds + 1) * EPS * blk(np.abs(v) + b)) / ds
