"""The three kernels of parallel-in-time sampling through ops on MI355X (afldm_amd/csrc/picard.hip) with synthetic eps, no UNet:
afldm_picard_sweep against chains of afldm_ddim_step on the same operands (torch.equal) and float64 errors, afldm_picard_stride
and afldm_picard_slide against the integer logic of tests/picard_oracle.py on planted partial sums, and the three together on
an eps that depends on the row only.

Shapes: (4, 16, 16) takes the 16-byte form (one block of 256 threads), (3, 5, 7) the scalar one (105 elements: a ragged block);
(4, 32, 32) more than one block (4).  Windows 1, 2, 5; 1 and 3 images; schedules of 1, 4 and 7 rows - at window 5 the 4-row
schedule ends inside the window.

Measured on MI355X: every swept row bit-identical to afldm_ddim_step's; the largest error of an err against float64 of the same
differences, as a share of the bound (E + 4) 2^-24: 1.5e-3 at (4, 16, 16), 1.7e-2 at (3, 5, 7), 4.2e-4 at (4, 32, 32)."""
import math

import pytest
import torch

import picard_oracle as po

pytestmark = pytest.mark.gpu

SHAPES = ((4, 16, 16), (3, 5, 7))
WINDOWS, IMAGES, ROWS = (1, 2, 5), (1, 3), (1, 4, 7)
T_WIDTH = {torch.float32: 4 * 13, torch.bfloat16: 8 * 13}             # a time-embedding row of 13 chunks of 16 bytes


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def _schedule(n):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    return ffhq_ddim_scheduler().schedule(n)


def _image(ident, Wn, shape):
    """(states [Wn + 1, C, H, W], eps [Wn, C, H, W]) of the image `ident`, whatever batch it is put in.  The states differ from
    each other by O(1), so no error is near zero."""
    g = torch.Generator().manual_seed(1000 + ident)
    return torch.randn((Wn + 1,) + shape, generator=g), torch.randn((Wn,) + shape, generator=g)


def _bases(P, n):
    """Cursors that meet the start, the last row (the window overruns the end) and, with 3 images, a finished one."""
    return [[0, n - 1, n][p % 3] for p in range(P)] if P > 1 else [0]


class Case:
    """Device buffers of one launch sequence: idents name the images, bases their cursors."""

    def __init__(self, shape, Wn, n, dtype, idents, bases, offset=0):
        from afldm_amd import ops
        self.shape, self.Wn, self.n, self.P, self.dtype = shape, Wn, n, len(idents), dtype
        P, E = self.P, math.prod(shape)
        imgs = [_image(i, Wn, shape) for i in idents]
        x = torch.stack([im[0] for im in imgs], 1)                         # [Wn + 1, P, C, H, W]
        e = torch.stack([im[1] for im in imgs], 1)                         # [Wn, P, C, H, W]
        flat = torch.zeros(x.numel() + offset, device="cuda")
        self.x = flat[offset:].view(x.shape)
        self.x.copy_(x)
        self.y = torch.full((Wn, P) + shape, float("nan"), device="cuda")
        self.eps = e.reshape((Wn * P,) + shape).permute(0, 2, 3, 1).contiguous().to(dtype).cuda()
        self.sched = _schedule(n)
        self.row_coef = self.sched.table("cuda").contiguous()
        self.row_t = torch.tensor(self.sched.timesteps, dtype=torch.float32, device="cuda")
        self.row_temb = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")     # row r -> table row n - 1 - r
        g = torch.Generator().manual_seed(5)
        self.table = torch.randn(n, T_WIDTH[dtype], generator=g).to(dtype).cuda()
        self.rows = torch.randn(Wn * P, T_WIDTH[dtype], generator=g).to(dtype).cuda()
        self.t_out = -torch.arange(1, Wn * P + 1, device="cuda").float()
        self.active = torch.full((Wn * P,), 7, dtype=torch.int32, device="cuda")
        self.cur = torch.tensor([bases, [3] * P], dtype=torch.int32, device="cuda")
        self.stride = torch.full((P,), -5, dtype=torch.int32, device="cuda")
        self.err = torch.full((P, Wn), -1.0, device="cuda")
        self.log = torch.full((8, P), -9, dtype=torch.int32, device="cuda")
        self.partial = torch.full((P, Wn, ops.picard_blocks(*shape)), float("nan"), device="cuda")
        self.E = E

    def sweep(self):
        from afldm_amd import ops
        return ops.picard_sweep(self.x, self.eps, self.y, self.partial, self.row_coef, self.cur[0])

    def decide(self, tol2, gather_only=False):
        from afldm_amd import ops
        return ops.picard_stride(self.partial, self.cur, self.stride, self.err, self.log, self.row_t, self.row_temb, self.t_out,
                                 self.active, self.table, self.rows, tol2, self.shape, gather_only=gather_only)

    def slide(self):
        from afldm_amd import ops
        return ops.picard_slide(self.x, self.y, self.stride)

    def chain(self, p, base):
        """Y[1 .. Wn] of image p as afldm_ddim_step computes them, one launch per row."""
        from afldm_amd import ops
        coef, out, y = self.row_coef.reshape(-1), [], self.x[0, p][None].clone()
        for j in range(self.Wn):
            if base + j < self.n:
                step = torch.tensor([base + j], dtype=torch.int32, device="cuda")
                y = ops.ddim_step(y, self.eps[j * self.P + p][None].contiguous(), coef, step)
            out.append(y[0].clone())
        return out


# ------------------------------------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES + ((4, 32, 32),))
def test_sweep_bits_inactive_rows_and_errors(shape, dtype):
    worst = 0.0
    for Wn in WINDOWS:
        for P in IMAGES:
            for n in ROWS:
                bases = _bases(P, n)
                c = Case(shape, Wn, n, dtype, list(range(P)), bases)
                x0 = c.x.clone()
                c.sweep()
                c.decide(float("inf"))
                assert torch.equal(_bits(c.x), _bits(x0)), "the sweep and the decision read the states only"
                err = c.err.cpu()
                for p, b in enumerate(bases):
                    if b >= n:                                             # finished: nothing of it is written
                        assert torch.isnan(c.y[:, p]).all() and torch.isnan(c.partial[p]).all() and (err[p] == -1).all()
                        continue
                    want = c.chain(p, b)
                    for j in range(Wn):
                        assert torch.equal(c.y[j, p], want[j]), (shape, Wn, P, n, p, j)
                        if b + j >= n:                                     # inactive: the copy of its predecessor, err exactly 0
                            assert torch.equal(c.y[j, p], c.y[j - 1, p] if j else c.x[0, p]) and float(err[p, j]) == 0.0
                            continue
                        ref = float((c.y[j, p].double() - x0[j + 1, p].double()).pow(2).mean())
                        assert ref > 0.1, "inputs whose errors are not near zero"
                        rel = abs(float(err[p, j]) - ref) / ref
                        worst = max(worst, rel / ((c.E + 4) * 2.0 ** -24))
                        assert rel <= (c.E + 4) * 2.0 ** -24, (shape, Wn, P, n, p, j, float(err[p, j]), ref)
    print(f"[picard] {shape} {dtype}: swept rows equal afldm_ddim_step's; worst err against float64: {worst:.3g} of (E + 4) 2^-24")


# ------------------------------------------------------------------------------------------------ 2. stride and slide
def _planted(Wn, n):
    """(base, [err_1 .. err_Wn] in units of tol^2) per image: all accepted, the first rejected, a middle one rejected, all accepted
    but the schedule ends inside the window, and a finished image."""
    lo, hi = 0.25, 4.0
    mid = (Wn + 1) // 2
    return [(0, [lo] * Wn), (0, [hi] + [lo] * (Wn - 1)), (0, [lo] * (mid - 1) + [hi] * (Wn - mid + 1)),
            (max(0, n - 2), [lo] * Wn), (n, [hi] * Wn)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_stride_slide_and_gather_on_planted_sums(shape, dtype):
    tol2 = 0.5
    for Wn in WINDOWS:
        for n in ROWS:
            cases = _planted(Wn, n)
            P = len(cases)
            bases = [b for b, _ in cases]
            c = Case(shape, Wn, n, dtype, list(range(P)), bases)
            c.y.copy_(torch.randn(c.y.shape, generator=torch.Generator().manual_seed(9)))
            nblk = c.partial.shape[2]
            for p, (b, errs) in enumerate(cases):
                for j in range(Wn):                                        # the sum over the blocks is err * tol^2 * E, to rounding
                    c.partial[p, j] = errs[j] * tol2 * c.E / nblk
            # the finished image: a planted bit pattern in its states and in its rows of the UNet's inputs (NaNs with a payload)
            fin = P - 1
            c.x.view(torch.int32)[:, fin] = 0x7FC12345
            before = {k: _bits(getattr(c, k)) for k in ("x", "rows", "t_out", "active")}
            c.decide(tol2)
            c.slide()
            want_s = [po.decide([e * tol2 for e in errs], b, n, Wn, tol2) for b, errs in cases]
            assert want_s[0] == min(Wn, n) and want_s[1] == 1 and want_s[2] == min(max(1, (Wn + 1) // 2), n) and want_s[4] == 0
            assert want_s[3] == min(Wn, n - bases[3]) and all(1 <= s <= Wn for s in want_s[:4])
            assert c.stride.cpu().tolist() == want_s, (Wn, n, c.stride.cpu().tolist(), want_s)
            cur = c.cur.cpu().tolist()
            assert cur[0] == [b + s for b, s in zip(bases, want_s)] and cur[1] == [4] * P
            log = c.log.cpu()
            assert log[3].tolist() == want_s and (log[:3] == -9).all() and (log[4:] == -9).all()
            y, x1 = c.y.cpu(), c.x.cpu()
            rows, t_out, active = _bits(c.rows), c.t_out.cpu(), c.active.cpu()
            for p, s in enumerate(want_s):
                us = [j * P + p for j in range(Wn)]
                if s == 0:                                                 # the same bits after the launches
                    for k in ("x", "rows", "t_out", "active"):
                        now = _bits(getattr(c, k))
                        sel = (slice(None), p) if k == "x" else (us,)
                        assert torch.equal(now[sel], before[k][sel]), (k, p)
                    continue
                for j in range(Wn + 1):
                    assert torch.equal(x1[j, p], y[min(j + s, Wn) - 1, p]), (Wn, n, p, j, s)
                for j, u in enumerate(us):
                    r = bases[p] + s + j
                    if r < n:
                        assert int(active[u]) == 1 and float(t_out[u]) == float(c.sched.timesteps[r])
                        assert torch.equal(rows[u], _bits(c.table)[n - 1 - r])
                    else:                                                  # past the end: flagged, and evaluated with what it held
                        assert int(active[u]) == 0 and torch.equal(rows[u], before["rows"][u])
                        assert torch.equal(_bits(t_out)[u], before["t_out"][u])


def test_gather_only_moves_no_cursor():
    c = Case((3, 5, 7), 2, 4, torch.float32, [0, 1, 2], [0, 3, 4])
    c.decide(0.0, gather_only=True)
    assert c.cur.cpu().tolist() == [[0, 3, 4], [3, 3, 3]] and c.stride.cpu().tolist() == [-5] * 3 and (c.log == -9).all()
    assert c.active.cpu().tolist() == [1, 1, 0, 1, 0, 0]
    assert c.t_out.cpu().tolist()[:2] == [float(c.sched.timesteps[0]), float(c.sched.timesteps[3])]
    assert c.t_out.cpu().tolist()[3] == float(c.sched.timesteps[1])


# ------------------------------------------------------------------------------------------------ 3. position invariance
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_an_image_does_not_depend_on_its_batch(shape, dtype):
    Wn, n, tol2 = 5, 7, 2.0                       # (errors of O(1) states are about 2: some rows pass, some do not)
    alone = Case(shape, Wn, n, dtype, [4], [1])
    among = Case(shape, Wn, n, dtype, [0, 1, 4], [0, 6, 1])
    for c in (alone, among):
        c.sweep()
        c.decide(tol2)
        c.slide()
    assert 1 <= int(alone.stride[0]) <= Wn
    for k in ("y", "x", "partial", "err", "stride"):
        a, b = getattr(alone, k), getattr(among, k)
        a, b = (a[0], b[2]) if k in ("partial", "err", "stride") else (a[:, 0], b[:, 2])
        assert torch.equal(_bits(a), _bits(b)), k
    assert int(alone.cur[0, 0]) == int(among.cur[0, 2])
    on = alone.active.bool().cpu()                 # (a row past the end keeps what its batch had planted there)
    assert torch.equal(alone.active, among.active[2::3]) and int(on.sum()) >= 1
    assert torch.equal(_bits(alone.rows)[on], _bits(among.rows[2::3])[on])
    assert torch.equal(alone.t_out.cpu()[on], among.t_out[2::3].cpu()[on])


# ------------------------------------------------------------------------------------------------ 4. the three launches together
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_row_only_eps_converges_in_one_sweep_per_window(shape, dtype):
    """eps depends on the row only, so ONE sweep computes the exact chain; at tolerance 0 a fresh window accepts one state (every
    estimate was a copy of the first) and the next iteration a whole window: picard_oracle.row_only_iterations, which is
    1 + ceil((n - 1) / W) up to n = W + 1 rows."""
    from afldm_amd import ops
    for Wn in WINDOWS:
        for P in IMAGES:
            for n in ROWS:
                c = Case(shape, Wn, n, dtype, list(range(P)), [0] * P)
                c.cur[1].zero_()
                c.x.copy_(c.x[0].clone()[None].expand_as(c.x))             # every state starts as the start latent
                start = c.x[0].clone()
                g = torch.Generator().manual_seed(77)
                by_row = torch.randn((n,) + shape, generator=g).permute(0, 2, 3, 1).contiguous().to(dtype).cuda()      # NHWC
                iters = 0
                while min(c.cur[0].cpu().tolist()) < n:
                    assert iters < n
                    base = c.cur[0].cpu().tolist()
                    for j in range(Wn):
                        for p in range(P):
                            c.eps[j * P + p] = by_row[min(base[p] + j, n - 1)]
                    c.sweep()
                    c.decide(0.0)
                    c.slide()
                    iters += 1
                assert iters == po.row_only_iterations(n, Wn), (Wn, P, n, iters)
                if n <= Wn + 1 or Wn == 1:
                    assert iters == 1 + math.ceil((n - 1) / Wn)
                coef = c.row_coef.reshape(-1)
                for p in range(P):
                    y = start[p][None].clone()
                    for r in range(n):
                        y = ops.ddim_step(y, by_row[r][None].contiguous(), coef, torch.tensor([r], dtype=torch.int32, device="cuda"))
                    assert torch.equal(c.x[0, p], y[0]), (Wn, P, n, p)


# ------------------------------------------------------------------------------------------------ 5. alignment
def test_misaligned_states():
    from afldm_amd._lib import AfldmError
    c = Case((4, 16, 16), 2, 4, torch.float32, [0], [0], offset=1)       # whole 16-byte groups, 4 bytes off: refused
    with pytest.raises(AfldmError, match="16-byte aligned"):
        c.sweep()
    with pytest.raises(AfldmError, match="16-byte aligned"):
        c.slide()
    off, on = (Case((3, 5, 7), 2, 4, torch.float32, [0], [0], offset=o) for o in (1, 0))       # the scalar form takes any address
    for c in (off, on):
        c.sweep()
        c.decide(1.0)
        c.slide()
    assert off.x.data_ptr() % 16 != 0 and torch.equal(off.x, on.x) and torch.equal(off.err, on.err)
