"""afldm_slot_step_kinds through ops on MI355X (afldm_amd/csrc/slot_kinds.hip, libafldm_slots.so): a batch whose slots walk "dpm" and "ddim" stretches of
one row table.  An active "dpm" slot must give afldm_dpm_step's bits on its own slices - x and both history planes - an active
"ddim" slot afldm_ddim_step's with its history untouched, a frozen slot nothing at all; tests/slot_dpm_oracle.py is the float64
check.  Shapes, slot states and `shift` as tests/test_gpu_slots.py; slot b walks stretch (b + shift // 2) % 2, so that with
B = 5 the two shifts put every state on a slot of each kind."""
import pytest
import torch

import slot_dpm_oracle as sdo
import slot_oracle as so
from test_gpu_slots import R, SPANS, T, _bits

pytestmark = pytest.mark.gpu

DPM, DDIM = 0, 1                # the stretches: rows 0 .. 6 are "dpm", rows 7 .. 11 "ddim"
NAMES = ("never started", "mid-schedule", "last row", "finished")


def _states(B, shift):
    """(pos, end, state, stretch) per slot: slot b in state (b + shift) % 4 on stretch (b + shift // 2) % 2."""
    pos, end, state, stretch = [], [], [], []
    for b in range(B):
        s, k = (b + shift) % 4, (b + shift // 2) % 2
        begin, stop = SPANS[k]
        pos.append([begin - 1, begin + 1, stop - 2, stop - 1][s])
        end.append(stop)
        state.append(s)
        stretch.append(k)
    return torch.tensor(pos, dtype=torch.int32), torch.tensor(end, dtype=torch.int32), state, stretch


def _tables(seed):
    """row_coef [R, 8], row_kind [R], row_t, row_temb: the "dpm" stretch's first row has b1 = b2 = 0, its second b2 = 0, the rest
    all six nonzero; a "ddim" row is four floats with c0 in [0.5, 1.5) and four zeros."""
    g = torch.Generator().manual_seed(seed)
    row_coef = torch.zeros(R, 8)
    (d0, d1), (c0, c1) = SPANS[DPM], SPANS[DDIM]
    row_coef[d0:d1, :6] = (torch.rand(d1 - d0, 6, generator=g) + 0.25) * torch.tensor([1, -1, 1, 1, -1, 1.0])
    row_coef[d0, 4:6] = 0.0
    row_coef[d0 + 1, 5] = 0.0
    row_coef[c0:c1, :4] = torch.rand(c1 - c0, 4, generator=g) + 0.5
    row_kind = torch.zeros(R, dtype=torch.int32)
    row_kind[d0:d1] = sdo.KIND_DPM
    row_t = torch.randint(0, 1000, (R,), generator=g).float()
    row_temb = torch.randint(0, T, (R,), generator=g).to(torch.int32)
    assert (row_coef[d0 + 2:d1, :6] != 0).all() and (row_coef[d0 + 1, :5] != 0).all() and (row_coef[d0, :4] != 0).all()
    return row_coef, row_kind, row_t, row_temb


def _dpm_step_of_slot(ops, x, eps, hist, row_coef, b, r):
    """ops.dpm_step on slot b's own slices with row r: -> (x_out, hist_out [2, 1, C, H, W])."""
    h = hist[:, b:b + 1].contiguous()
    idx = torch.tensor([r], dtype=torch.int32, device="cuda")
    out = ops.dpm_step(x[b:b + 1].contiguous(), eps[b:b + 1].contiguous(), h, row_coef.reshape(-1), idx)
    return out, h


def _step_case(B, C, H, W, dtype, shift):
    from afldm_amd import ops
    row_coef, row_kind, row_t, row_temb = _tables(3)
    pos, end, state, stretch = _states(B, shift)
    pos, _, active, _ = so.select(row_t, row_temb, pos, end, torch.zeros(B), torch.zeros(T, 4), torch.zeros(B, 4))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, C, H, W, generator=g)
    eps = torch.randn(B, H, W, C, generator=g).to(dtype)
    hist = torch.randn(2, B, C, H, W, generator=g)
    for b in range(B):
        if not int(active[b]):                                             # neither read nor written: NaN in, the same bits out
            eps[b] = float("nan")
            x[b, 0, 0, 0] = float("nan")
            hist[:, b, 0, 0, 0] = float("nan")
    xd, ed, hd, cd, kd, pd, ad = (v.cuda() for v in (x, eps, hist, row_coef, row_kind, pos, active))
    want_x, want_h = xd.clone(), hd.clone()
    for b in range(B):
        if not int(active[b]):
            continue
        if stretch[b] == DPM:
            out, h = _dpm_step_of_slot(ops, xd, ed, hd, cd, b, int(pos[b]))
            want_x[b:b + 1], want_h[:, b:b + 1] = out, h
        else:
            idx = torch.tensor([int(pos[b])], dtype=torch.int32, device="cuda")
            ddim_coef = cd[:, :4].contiguous().reshape(-1)
            want_x[b:b + 1] = ops.ddim_step(xd[b:b + 1].contiguous(), ed[b:b + 1].contiguous(), ddim_coef, idx)
    got_x, got_h = xd.clone(), hd.clone()
    assert ops.slot_step_kinds(got_x, ed, got_h, cd, kd, pd, ad) is got_x
    live = [stretch[b] for b in range(B) if int(active[b])]
    assert live and (int(active.sum()) < B) == (B == 5 or shift == 2)
    if B == 5:
        assert DPM in live and DDIM in live and int(active.sum()) < B, "an active slot of each kind and a frozen one"
        covered = {pair for s in (0, 2) for pair in zip(*_states(5, s)[2:])}
        assert covered == {(s, k) for s in range(4) for k in (DPM, DDIM)}, "the two shifts put every state on a slot of each kind"
    for b in range(B):
        what = f"slot {b} ({NAMES[state[b]]}, {'dpm' if stretch[b] == DPM else 'ddim'})"
        assert torch.equal(_bits(got_x[b]), _bits(want_x[b])), what + ": x must have the plain step kernel's bits"
        assert torch.equal(_bits(got_h[:, b]), _bits(want_h[:, b])), what + ": history"
        if not int(active[b]) or stretch[b] == DDIM:
            assert torch.equal(_bits(got_h[:, b]), _bits(hist[:, b])), what + ": history bit-unchanged"
        if not int(active[b]):
            assert torch.equal(_bits(got_x[b]), _bits(x[b])), what + ": x bit-unchanged"
    assert torch.equal(pd.cpu(), pos) and torch.equal(ad.cpu(), active)
    ref_x, ref_h = sdo.step_kinds(x, eps.float().permute(0, 3, 1, 2), hist, row_coef, row_kind, pos, active)
    for b in range(B):
        if int(active[b]):
            pairs = [(got_x[b], ref_x[b])] + ([(got_h[0, b], ref_h[0, b]), (got_h[1, b], ref_h[1, b])] if stretch[b] == DPM else [])
            for got, ref in pairs:
                err = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
                assert err <= 1e-5, (b, err)


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("plane", [5, 16])                                # HW = 25: the scalar form; 256: the 16-byte form
@pytest.mark.parametrize("B", [3, 5])
def test_step_kinds(B, plane, dtype, shift):
    _step_case(B, 4, plane, plane, dtype, shift)


def test_step_kinds_beyond_one_grid():
    """C H W = 4 * 363^2 = 527076 > 2048 * 256: the grid-stride loop runs a second pass (scalar form, HW odd)."""
    _step_case(3, 4, 363, 363, torch.bfloat16, 0)


# ------------------------------------------------------------------------------------------------ a stale history
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("plane", [5, 16])
def test_stale_history_reaches_nothing(plane, dtype):
    """Slot 1 is refilled on a history full of NaN and Inf and runs its first three rows, one select between each: x after
    every row, and both planes after the third, are three afldm_dpm_step calls from a cleared history, bit for bit."""
    from afldm_amd import ops
    B, C = 3, 4
    row_coef, row_kind, row_t, row_temb = _tables(6)
    begin, stop = SPANS[DPM]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, plane, plane, generator=g)
    hist = torch.full((2, B, C, plane, plane), float("nan"))
    hist[:, :, :, ::2] = float("inf")
    hist[1, :, 1] = -float("inf")
    pos = torch.tensor([stop - 1, begin - 1, SPANS[DDIM][1] - 1], dtype=torch.int32)          # slots 0 and 2 have finished
    end = torch.tensor([stop, stop, SPANS[DDIM][1]], dtype=torch.int32)
    d = dict(row_t=row_t, row_temb=row_temb, pos=pos, end=end, t_out=torch.zeros(B), active=torch.zeros(B, dtype=torch.int32),
             table=torch.zeros(T, 4), rows=torch.zeros(B, 4))
    d = {k: v.cuda() for k, v in d.items()}
    xd, hd, cd, kd = x.cuda(), hist.cuda(), row_coef.cuda(), row_kind.cuda()
    want_x, want_h = xd[1:2].clone(), torch.zeros(2, 1, C, plane, plane, device="cuda")
    for k in range(3):
        eps = torch.randn(B, plane, plane, C, generator=g).to(dtype).cuda()
        ops.slot_select(d["row_t"], d["row_temb"], d["pos"], d["end"], d["t_out"], d["active"], d["table"], d["rows"])
        assert d["pos"].cpu().tolist() == [stop - 1, begin + k, SPANS[DDIM][1] - 1] and d["active"].cpu().tolist() == [0, 1, 0]
        ops.slot_step_kinds(xd, eps, hd, cd, kd, d["pos"], d["active"])
        idx = torch.tensor([begin + k], dtype=torch.int32, device="cuda")
        want_x = ops.dpm_step(want_x, eps[1:2].contiguous(), want_h, cd.reshape(-1), idx)
        assert torch.isfinite(want_x).all()
        assert torch.equal(_bits(xd[1:2]), _bits(want_x)), f"row {k}: x"
    assert torch.equal(_bits(hd[:, 1:2]), _bits(want_h)), "both planes after the third row"
    for b in (0, 2):                                                       # the finished neighbours: nothing moved
        assert torch.equal(_bits(xd[b]), _bits(x[b])) and torch.equal(_bits(hd[:, b]), _bits(hist[:, b]))


# ------------------------------------------------------------------------------------------------ edges
def test_out_of_range_indices_skip_the_slot():
    """A kind code that is neither 0 nor 1, and a pos of R, leave their slots bit-unchanged; the slot between them is updated."""
    from afldm_amd import ops
    B, C, plane = 3, 4, 16
    row_coef, row_kind, _, _ = _tables(8)
    row_kind[SPANS[DPM][0] + 3] = 7
    g = torch.Generator().manual_seed(9)
    x, hist = torch.randn(B, C, plane, plane, generator=g), torch.randn(2, B, C, plane, plane, generator=g)
    eps = torch.randn(B, plane, plane, C, generator=g)
    pos = torch.tensor([SPANS[DPM][0] + 3, SPANS[DPM][0] + 4, R], dtype=torch.int32)
    active = torch.ones(B, dtype=torch.int32)
    xd, ed, hd, cd, kd, pd, ad = (v.cuda() for v in (x, eps, hist, row_coef, row_kind, pos, active))
    want_x, want_h = _dpm_step_of_slot(ops, xd, ed, hd, cd, 1, int(pos[1]))
    ops.slot_step_kinds(xd, ed, hd, cd, kd, pd, ad)
    for b in (0, 2):
        assert torch.equal(_bits(xd[b]), _bits(x[b])) and torch.equal(_bits(hd[:, b]), _bits(hist[:, b])), b
    assert torch.equal(_bits(xd[1:2]), _bits(want_x)) and torch.equal(_bits(hd[:, 1:2]), _bits(want_h))
    pd.fill_(-1)                                                           # below the table as well
    before_x, before_h = xd.clone(), hd.clone()
    ops.slot_step_kinds(xd, ed, hd, cd, kd, pd, ad)
    assert torch.equal(_bits(xd), _bits(before_x)) and torch.equal(_bits(hd), _bits(before_h))


def test_bad_arguments_are_errors():
    from afldm_amd import _lib, _slots, ops
    lib, P, st = _slots.lib(), _lib.ptr, _lib.stream_ptr()
    ENULL, ESHAPE, EDTYPE = -5, -1, -2
    B, C, plane = 2, 4, 4
    x, hist = torch.randn(B, C, plane, plane).cuda(), torch.randn(2, B, C, plane, plane).cuda()
    eps = torch.randn(B, plane, plane, C).cuda()
    coef, kind = torch.rand(R, 8).cuda(), torch.ones(R, dtype=torch.int32).cuda()
    pos, active = torch.zeros(B, dtype=torch.int32).cuda(), torch.ones(B, dtype=torch.int32).cuda()
    keep = [t.clone() for t in (x, hist)]

    def call(**over):
        a = dict(x=P(x), eps=P(eps), hist=P(hist), coef=P(coef), kind=P(kind), pos=P(pos), active=P(active), B=B, R=R, C=C,
                 H=plane, W=plane, dtype=_lib.F32)
        a.update(over)
        return lib.afldm_slot_step_kinds(a["x"], a["eps"], a["hist"], a["coef"], a["kind"], a["pos"], a["active"], a["B"], a["R"],
                                         a["C"], a["H"], a["W"], a["dtype"], st)
    for name in ("x", "eps", "hist", "coef", "kind", "pos", "active"):
        assert call(**{name: None}) == ENULL, name
    for over in (dict(B=0), dict(B=65536), dict(R=0), dict(C=-1), dict(H=0), dict(W=0), dict(C=1 << 15, H=1 << 8, W=1 << 8)):
        assert call(**over) == ESHAPE, over
    assert call(dtype=7) == EDTYPE and b"afldm_slot_step_kinds" in _lib.lib.afldm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, keep[0]) and torch.equal(hist, keep[1])          # no refused call wrote anything
    with pytest.raises(RuntimeError, match="cuda"):
        ops.slot_step_kinds(torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4, 4), torch.zeros(2, 2, 4, 4, 4), torch.zeros(R, 8),
                            torch.zeros(R, dtype=torch.int32), pos, active)
