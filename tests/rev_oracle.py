"""numpy restatement of the bit-reversible sampler's arithmetic (afldm_rev_encode, afldm_rev_step in include/afldm_hip.h): the
fp32 operations one by one - numpy never fuses a multiply with an add - and int64 adds with overflow detection.  The GPU tests
compare the kernels with this bit for bit; tests/test_rev_host.py runs it on its own invariants."""
import numpy as np

F = np.float32
UP, DOWN = F(2.0 ** 32), F(2.0 ** -32)


def encode(x):
    """fp32 x -> (int64 rn(x 2^32), trouble per element): a non-finite x or |x| >= 2^31 gives 0 and trouble."""
    x = np.asarray(x, dtype=F)
    bad = ~np.isfinite(x) | (np.abs(x) >= F(2.0 ** 31))
    with np.errstate(all="ignore"):
        v = np.where(bad, F(0), x) * UP          # exact
    return np.rint(v).astype(np.int64), bad


def decode(X):
    """rn_f32(X) 2^-32: one int64 -> fp32 rounding (to nearest even), then an exact scale."""
    return np.asarray(X, dtype=np.int64).astype(F) * DOWN


def step(far, near, eps, row):
    """(far, near, eps, (cx, ce, sign, boot)) -> (new far, new near, lat, trouble per element)."""
    cx, ce, sign, boot = F(row[0]), F(row[1]), int(row[2]), bool(row[3])
    assert sign in (1, -1)
    far, near = np.asarray(far, dtype=np.int64), np.asarray(near, dtype=np.int64)
    f = near if boot else far
    with np.errstate(all="ignore"):
        x = decode(near)
        a = cx * x
        b = ce * np.asarray(eps, dtype=F)
        d = a + b
        v = d * UP
        ok = np.isfinite(d) & (np.abs(v) < F(2.0 ** 63))
        q = np.rint(np.where(ok, v, F(0))).astype(np.int64)
        sq = -q if sign < 0 else q
        new = f + sq                                         # wraps; overflow: both operands differ in sign from the sum
    over = ((f ^ new) & (sq ^ new)) < 0
    new = np.where(over, f, new)
    assert a.dtype == b.dtype == d.dtype == v.dtype == F and new.dtype == np.int64
    return near.copy(), new, decode(new), ~ok | over


def run(rows, timesteps, eps_fn, near, far=None):
    """The loop: (far, near) through the rows, eps_fn(lat fp32, t) -> eps.  Returns the list of `near` after every row and the
    final far; raises FloatingPointError on trouble."""
    near = np.asarray(near, dtype=np.int64)
    far = near.copy() if far is None else np.asarray(far, dtype=np.int64)
    states = []
    for t, row in zip(timesteps, rows):
        far, near, _, bad = step(far, near, eps_fn(decode(near), t), row)
        if bad.any():
            raise FloatingPointError("trouble")
        states.append(near)
    return states, far


def f32_rows(sched):
    """A Schedule's rows as the device table has them: rounded once to fp32."""
    return [tuple(float(v) for v in r) for r in sched.table("cpu").tolist()]
