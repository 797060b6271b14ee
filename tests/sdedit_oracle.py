"""Image-to-image sampling (SDEdit with a change map) restated in float64 torch: what tests/test_sdedit_host.py checks on its own
invariants and the GPU tests compare afldm_sdedit_step and MyLDMPipeline.img2img_latents against.

The coefficients are the ones the kernel reads: Schedule.table's fp32-rounded rows, widened to float64.  The threshold a change
value is compared with is then the same bit pattern on both sides, so no element near a threshold has to be left out of a
comparison: the select falls the same way here and on the GPU."""
import torch


def f32(values):
    """Python floats as the kernel gets them: rounded once to fp32, then widened."""
    return [float(v) for v in torch.tensor([float(v) for v in values], dtype=torch.float64).to(torch.float32)]


def rows_of(schedule):
    """Schedule.table's rows as lists of floats (fp32 values)."""
    return [[float(v) for v in r] for r in schedule.table("cpu").double()]


def sdedit_step(x, e, orig, cmap, z, zu, row):
    """One update on float64 tensors; row = (p, q, lo, hi, a, b, c, k0, k1, thr, ...) as fp32 values.  cmap broadcasts against x
    ([B | 1, 1, H, W] or x's shape).  z is not looked at where k1 = 0, zu not where c = 0.  A select: what the other side holds at
    an element - a NaN included - does not reach the result, and a NaN in cmap compares false (generated)."""
    p, q, lo, hi, a, b, c, k0, k1, thr = [float(v) for v in row[:10]]
    x, e, orig, cmap = x.double(), e.double(), orig.double(), cmap.double()
    xp = a * torch.clamp(p * x + q * e, lo, hi) + b * e
    if c != 0.0:
        xp = xp + c * zu.double()
    held = k0 * orig
    if k1 != 0.0:
        held = held + k1 * z.double()
    return torch.where((cmap <= thr).expand_as(x), held, xp)


def start_row(k0, k1):
    """The row whose update is the start of a run: everything held at k0 orig + k1 z."""
    inf = float("inf")
    return (0.0, 0.0, -inf, inf, 0.0, 0.0, 0.0, k0, k1, inf)


def x_start(orig, z, start):
    k0, k1 = f32(start)
    return k0 * orig.double() + k1 * z.double()


def reverse_step(x, e, zu, row):
    """The reverse step alone: the first seven fields of the row."""
    p, q, lo, hi, a, b, c = [float(v) for v in row[:7]]
    xp = a * torch.clamp(p * x.double() + q * e.double(), lo, hi) + b * e.double()
    return xp + c * zu.double() if c != 0.0 else xp


def sample(eps, orig, cmap, z, schedule, start, draw=None, trace=None):
    """The whole loop in float64 around a callable eps(x, t) -> tensor: x_start = k0_start orig + k1_start z, then one sdedit_step
    per evaluation; draw() is called once per evaluation the schedule draws at, in order.  trace: a list that receives the state
    after every evaluation."""
    x = x_start(orig, z, start)
    for k, (t, row) in enumerate(zip(schedule.timesteps, rows_of(schedule))):
        e = eps(x, t)
        zu = draw() if schedule.slots(k) else None
        x = sdedit_step(x, e, orig, cmap, z, zu, row)
        if trace is not None:
            trace.append(x.clone())
    return x


def sample_plain(eps, x, schedule, draw=None):
    """The plain truncated reverse loop over the same rows from a given start: what an element of change value 1 follows."""
    x = x.double()
    for k, (t, row) in enumerate(zip(schedule.timesteps, rows_of(schedule))):
        e = eps(x, t)
        x = reverse_step(x, e, draw() if schedule.slots(k) else None, row)
    return x
