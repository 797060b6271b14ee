"""The slot sampler's three kernels through ops on MI355X (afldm_amd/csrc/slots.hip) against tests/slot_oracle.py: everything
they move is compared with torch.equal - the kernels copy, count, and apply afldm_ddim_step's update bit for bit.

Slots are put in the four states a step can meet: never started (pos = begin - 1), mid-schedule, about to run its last row
(pos = end - 2), and already finished (pos = end - 1).  `shift` rotates the assignment so that a batch of 3 meets all four."""
import pytest
import torch

import slot_oracle as so

pytestmark = pytest.mark.gpu

R, T = 12, 6                    # two stretches of the row table: rows 0 .. 6 and 7 .. 11
SPANS = ((0, 7), (7, 12))


def _states(B, shift):
    """(pos, end) int32 [B]: slot b in state (b + shift) % 4 on stretch b % 2."""
    pos, end = [], []
    for b in range(B):
        begin, stop = SPANS[b % 2]
        pos.append([begin - 1, begin + 1, stop - 2, stop - 1][(b + shift) % 4])
        end.append(stop)
    return torch.tensor(pos, dtype=torch.int32), torch.tensor(end, dtype=torch.int32)


def _tables(seed):
    g = torch.Generator().manual_seed(seed)
    row_coef = torch.rand(R, 4, generator=g) + 0.5                         # c0 in [0.5, 1.5): no division by ~0
    row_t = torch.randint(0, 1000, (R,), generator=g).float()
    row_temb = torch.randint(0, T, (R,), generator=g).to(torch.int32)
    return row_coef, row_t, row_temb


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


# ------------------------------------------------------------------------------------------------ 1. select
@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("row_bytes", [16, 16 * (256 + 37)])          # one chunk; more than one pass of the workgroup's 256, ragged
@pytest.mark.parametrize("B", [3, 5])
def test_select(B, row_bytes, dtype, shift):
    from afldm_amd import ops
    width = row_bytes // torch.empty(0, dtype=dtype).element_size()
    _, row_t, row_temb = _tables(1)
    pos, end = _states(B, shift)
    g = torch.Generator().manual_seed(2)
    table = torch.randn(T, width, generator=g).to(dtype)
    rows = torch.randn(B, width, generator=g).to(dtype)                    # what the slots held before: a frozen slot keeps it
    t_out = -torch.arange(1, B + 1).float()
    want_pos, want_t, want_active, want_rows = so.select(row_t, row_temb, pos, end, t_out, table, rows)
    assert int(want_active.sum()) >= 1 and (int(want_active.sum()) < B) == (B == 5 or shift == 2)      # frozen slots among them
    d = [v.cuda() for v in (row_t, row_temb, pos, end, t_out, torch.full((B,), 7, dtype=torch.int32), table, rows)]
    ops.slot_select(*d)
    got_pos, got_end, got_t, got_active, got_rows = d[2].cpu(), d[3].cpu(), d[4].cpu(), d[5].cpu(), d[7].cpu()
    assert torch.equal(got_pos, want_pos) and torch.equal(got_end, end)
    assert torch.equal(got_t, want_t) and torch.equal(got_active, want_active)
    assert torch.equal(_bits(got_rows), _bits(want_rows))
    for b in range(B):
        if not int(want_active[b]):                                        # frozen: its timestep and its row bit-unchanged
            assert got_t[b] == t_out[b] and torch.equal(_bits(got_rows[b]), _bits(rows[b])) and got_pos[b] == pos[b]
    # two more prologues: the slots on their last row finish, and a finished slot is left alone from then on
    ops.slot_select(*d)
    ops.slot_select(*d)
    w2 = so.select(row_t, row_temb, want_pos, end, want_t, table, want_rows)
    w3 = so.select(row_t, row_temb, w2[0], end, w2[1], table, w2[3])
    assert torch.equal(d[2].cpu(), w3[0]) and torch.equal(d[4].cpu(), w3[1]) and torch.equal(d[5].cpu(), w3[2])
    assert torch.equal(_bits(d[7].cpu()), _bits(w3[3]))


# ------------------------------------------------------------------------------------------------ 2. step
def _step_case(B, C, H, W, dtype, shift):
    from afldm_amd import ops
    row_coef, row_t, row_temb = _tables(3)
    pos, end = _states(B, shift)
    pos, _, active, _ = so.select(row_t, row_temb, pos, end, torch.zeros(B), torch.zeros(T, 4), torch.zeros(B, 4))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, C, H, W, generator=g)
    eps = torch.randn(B, H, W, C, generator=g).to(dtype)
    for b in range(B):
        if not int(active[b]):                                             # neither read nor written: NaN in, the same bits out
            eps[b] = float("nan")
            x[b, 0, 0, 0] = float("nan")
    xd, ed, cd, pd, ad = x.cuda(), eps.cuda(), row_coef.cuda(), pos.cuda(), active.cuda()
    want = xd.clone()
    for b in range(B):
        if int(active[b]):
            idx = torch.tensor([int(pos[b])], dtype=torch.int32, device="cuda")
            want[b:b + 1] = ops.ddim_step(xd[b:b + 1].contiguous(), ed[b:b + 1].contiguous(), cd.reshape(-1), idx)
    got = ops.slot_step(xd.clone(), ed, cd, pd, ad)
    assert int(active.sum()) >= 1 and (int(active.sum()) < B) == (B == 5 or shift == 2)
    assert torch.equal(_bits(got), _bits(want)), "a slot must give afldm_ddim_step's bits for the same row"
    assert torch.equal(pd.cpu(), pos) and torch.equal(ad.cpu(), active)
    ref = so.step(x, eps.float().permute(0, 3, 1, 2), row_coef, pos, active)
    for b in range(B):
        if int(active[b]):
            err = float((got[b].cpu().double() - ref[b]).abs().max() / ref[b].abs().max())
            assert err <= 1e-5, (b, err)
        else:
            assert torch.equal(_bits(got[b]), _bits(x[b]))


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("plane", [5, 16])                                # HW = 25: the scalar form; 256: the 16-byte form
@pytest.mark.parametrize("B", [3, 5])
def test_step(B, plane, dtype, shift):
    _step_case(B, 4, plane, plane, dtype, shift)


def test_step_beyond_one_grid():
    """C H W = 4 * 363^2 = 527076 > 2048 * 256: the grid-stride loop runs a second pass (scalar form, HW odd)."""
    _step_case(3, 4, 363, 363, torch.bfloat16, 0)


# ------------------------------------------------------------------------------------------------ 3. exchange
def _exchange_case(B, C, H, W, cmd):
    from afldm_amd import ops
    g = torch.Generator().manual_seed(5)
    lat, out, fresh = (torch.randn(n, C, H, W, generator=g) for n in (B, 4, 2))
    lat[0, 0, 0, 0] = float("nan")                                         # copies are bit copies
    pos, end = _states(B, 1)
    cmd = torch.tensor(cmd, dtype=torch.int32)
    want = so.exchange(cmd, lat, out, fresh, pos, end)
    d = [v.cuda() for v in (cmd, lat, out, fresh, pos, end)]
    ops.slot_exchange(*d)
    for got, ref, name in zip((d[1], d[2], d[4], d[5]), want, ("lat", "out", "pos", "end")):
        assert torch.equal(_bits(got), _bits(ref)), name
    assert torch.equal(_bits(d[3]), _bits(fresh)) and torch.equal(d[0].cpu(), cmd)
    return lat, out, fresh, pos, end, [v.cpu() for v in (d[1], d[2], d[4], d[5])]


@pytest.mark.parametrize("C,plane", [(4, 5), (4, 16), (3, 5)])            # (3, 5): 75 floats per slot, the scalar form
@pytest.mark.parametrize("B", [3, 5])
def test_exchange(B, C, plane):
    idle = [-1, -1, 9, 9]
    # harvest only, refill only, both on one slot
    cmd = [[1, -1, 0, 0], [-1, 0, 7, 12], [0, 1, 0, 7]] + [idle] * (B - 3)
    lat, out, fresh, pos, end, (glat, gout, gpos, gend) = _exchange_case(B, C, plane, plane, cmd)
    assert torch.equal(_bits(gout[1]), _bits(lat[0])) and torch.equal(_bits(glat[0]), _bits(lat[0]))      # harvest only
    assert gpos[0] == pos[0] and gend[0] == end[0]
    assert torch.equal(glat[1], fresh[0]) and (int(gpos[1]), int(gend[1])) == (6, 12)                      # refill only
    assert torch.equal(gout[0], lat[2]) and torch.equal(glat[2], fresh[1])                                # both: the OLD latents leave
    assert (int(gpos[2]), int(gend[2])) == (-1, 7)
    assert torch.equal(gout[2:], out[2:])
    for b in range(3, B):                                                  # untouched slots
        assert torch.equal(glat[b], lat[b]) and gpos[b] == pos[b] and gend[b] == end[b]
    # nothing commanded: nothing moves
    _exchange_case(B, C, plane, plane, [idle] * B)


def test_exchange_beyond_one_grid():
    """C H W = 5 * 363^2 = 658845 > 2048 * 256, and odd: the scalar form's grid-stride loop runs a second pass."""
    _exchange_case(3, 5, 363, 363, [[1, -1, 0, 0], [-1, 0, 7, 12], [0, 1, 0, 7]])


def test_bad_arguments_are_errors():
    from afldm_amd import ops
    from afldm_amd._lib import AfldmError
    i32 = dict(dtype=torch.int32, device="cuda")
    pos, end, active = torch.zeros(2, **i32), torch.zeros(2, **i32), torch.zeros(2, **i32)
    row_t, row_temb, t_out = torch.zeros(R, device="cuda"), torch.zeros(R, **i32), torch.zeros(2, device="cuda")
    with pytest.raises(AfldmError, match="16-byte"):
        ops.slot_select(row_t, row_temb, pos, end, t_out, active, torch.zeros(T, 3, device="cuda"), torch.zeros(2, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="cuda"):
        ops.slot_step(torch.zeros(2, 4, 4, 4), torch.zeros(2, 4, 4, 4), torch.zeros(R, 4), pos, active)
