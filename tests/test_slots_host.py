"""The slot sampler's host side without a GPU: SamplingServer (afldm_amd/serving.py) and SlotTable (afldm_amd/engine.py) against
an engine that only counts.  The fake keeps the device's state as tests/slot_oracle.py restates it: a step advances every
active slot's cursor, adds 1 to channel 0 of its latents and the row's timestep to channel 1 - so a result says how many
evaluations its request got and at which timesteps, whatever shared its batch."""
import math
import types

import pytest
import torch

import slot_oracle as so

LENGTHS = (3, 5, 2, 4, 3, 5, 1, 2, 5, 4, 3, 2, 5, 1, 1, 4, 2, 3, 5, 2, 4, 3, 1)


class _Done:
    def query(self):
        return True

    def synchronize(self):
        pass


class CountingEngine:
    def __init__(self, B, steps_per_graph, row_capacity=1024, temb_capacity=256, out_capacity=None):
        from afldm_amd.engine import SlotTable
        self.B, self.steps_per_graph = B, steps_per_graph
        self.table = SlotTable(row_capacity, temb_capacity)
        self.out_capacity = 2 * B if out_capacity is None else out_capacity
        self.lat = torch.zeros(B, 2, 1, 1, dtype=torch.float64)
        self.out = torch.zeros(self.out_capacity, 2, 1, 1, dtype=torch.float64)
        self.pos, self.end = torch.full((B,), -1, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        self.replays, self.groups, self.refilled, self.launches = 0, [], [], 0
        self.before_step = None

    def add_schedule(self, schedule):
        return self.table.add(schedule)

    def refresh_if_stale(self):
        return False

    def check_errors(self):
        pass

    def remaining(self):
        return [max(0, int(e) - int(p) - 1) for p, e in zip(self.pos, self.end)]

    def exchange(self, harvests, refills):
        if not harvests and not refills:
            return {}
        self.launches += 1
        cmd = torch.full((self.B, 4), -1, dtype=torch.int32)
        fresh = torch.zeros_like(self.lat)
        for i, (b, (z, begin, end)) in enumerate(refills.items()):
            cmd[b, 1:] = torch.tensor([i, begin, end], dtype=torch.int32)
            fresh[i] = z.reshape(2, 1, 1)
            self.refilled.append((b, float(z.reshape(-1)[0])))
        for b, idx in harvests.items():
            assert 0 <= idx < self.out_capacity
            cmd[b, 0] = idx
        self.lat, self.out, self.pos, self.end = so.exchange(cmd, self.lat, self.out, fresh, self.pos, self.end)
        return {b: _Done() for b in harvests}

    def take(self, idx):
        return self.out[idx].clone().unsqueeze(0)

    def step(self, k):
        if self.before_step is not None:
            self.before_step(k)
        self.groups.append(k)
        self.replays += k // self.steps_per_graph + k % self.steps_per_graph
        row_t = torch.tensor(self.table.t, dtype=torch.float64)
        for _ in range(k):
            for b in range(self.B):
                if int(self.pos[b]) + 1 < int(self.end[b]):
                    self.pos[b] += 1
                    self.lat[b, 0] += 1
                    self.lat[b, 1] += row_t[int(self.pos[b])]


def _pipe():
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = types.SimpleNamespace(config=types.SimpleNamespace(in_channels=2, sample_size=1), device=torch.device("cpu"),
                                 dtype=torch.float32)
    return types.SimpleNamespace(unet=unet, scheduler=ffhq_ddim_scheduler())


def _server(slots, steps_per_graph, engines=1, **kw):
    from afldm_amd.serving import SamplingServer
    return SamplingServer(_pipe(), slots, steps_per_graph, engines,
                          engine_factory=lambda i: CountingEngine(slots, steps_per_graph, **kw))


def _submit_all(server, lengths):
    # request i starts from (1000 i, 0): channel 0 ends at 1000 i + its step count, channel 1 at the sum of its timesteps
    return [server.submit(n, latents=torch.tensor([1000.0 * i, 0.0]).reshape(1, 2, 1, 1)) for i, n in enumerate(lengths)]


def _check_results(tickets, lengths):
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    for i, (ticket, n) in enumerate(zip(tickets, lengths)):
        got = ticket.result()
        assert tuple(got.shape) == (1, 2, 1, 1) and ticket.done() and ticket.index == i
        assert float(got[0, 0]) == 1000.0 * i + n, (i, n, got)
        assert float(got[0, 1]) == float(sum(ffhq_ddim_scheduler().schedule(n).timesteps)), (i, n)


# ------------------------------------------------------------------------------------------------ 1. bookkeeping
@pytest.mark.parametrize("steps_per_graph", [1, 2, 3])
def test_mirror_refill_order_and_request_order_results(steps_per_graph):
    server = _server(4, steps_per_graph)
    eng = server.engines[0]
    tickets = _submit_all(server, LENGTHS)
    with pytest.raises(RuntimeError, match="not sampled yet"):
        tickets[0].result()
    assert not tickets[0].done()
    while server.poll(max_replays=1):
        # the mirror is the device's state, slot for slot (a slot the host has emptied is finished on the device)
        mirror = [0 if s is None else s[1] for s in server._slot[0]]
        assert mirror == eng.remaining(), (mirror, eng.remaining())
    server.run()
    _check_results(tickets, LENGTHS)
    # refills in arrival order; the first boundary fills slots 0 .. 3 in order
    assert [start for _, start in eng.refilled] == [1000.0 * i for i in range(len(LENGTHS))]
    assert [b for b, _ in eng.refilled[:4]] == [0, 1, 2, 3]
    assert server.useful == sum(LENGTHS) and server.evaluations == 4 * sum(eng.groups) and server.replays == eng.replays
    assert all(s is None for s in server._slot[0]) and not server._queue[0] and not server._pending[0]
    assert sorted(server._free[0]) == list(range(eng.out_capacity))
    launches = eng.launches
    assert server.poll() == 0 and eng.launches == launches          # nothing changes: nothing is launched


def test_a_full_output_ring_waits_for_the_oldest_ticket():
    server = _server(4, 2, out_capacity=1)
    tickets = _submit_all(server, LENGTHS)
    server.run()
    _check_results(tickets, LENGTHS)


def test_two_engines_take_alternate_requests():
    server = _server(2, 2, engines=2)
    tickets = _submit_all(server, LENGTHS[:9])
    assert [t.engine for t in tickets] == [i % 2 for i in range(9)]
    server.run()
    _check_results(tickets, LENGTHS[:9])
    for e, eng in enumerate(server.engines):
        assert [start for _, start in eng.refilled] == [1000.0 * i for i in range(e, 9, 2)]


def test_add_schedule_deduplicates_and_shares_timestep_rows():
    from afldm_amd.engine import SlotTable
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    tb = SlotTable(64, 32)
    s5, s10 = ffhq_ddim_scheduler().schedule(5), ffhq_ddim_scheduler().schedule(10)
    assert tb.add(s5) == (0, 5) and tb.add(s10) == (5, 15)
    assert tb.add(ffhq_ddim_scheduler().schedule(5)) == (0, 5) and len(tb.t) == 15          # keyed on schedule.key: stored once
    distinct = set(s5.timesteps) | set(s10.timesteps)
    assert len(tb.timesteps) == len(set(tb.timesteps)) == len(distinct) < 15                  # the 5-step timesteps are shared
    assert [tb.timesteps[i] for i in tb.temb] == list(s5.timesteps) + list(s10.timesteps)
    assert tb.t == [float(t) for t in s5.timesteps + s10.timesteps] and tb.coef == list(s5.rows + s10.rows)


def test_full_tables_and_other_kinds_raise():
    from afldm_amd.engine import SlotTable
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    s5, s3, s7 = (ffhq_ddim_scheduler().schedule(n) for n in (5, 3, 7))
    tb = SlotTable(7, 32)
    tb.add(s5)
    with pytest.raises(RuntimeError, match="row table is full"):
        tb.add(s3)
    assert len(tb.t) == 5 and len(tb.timesteps) == 5 and s3.key not in tb.spans          # a refused schedule leaves no trace
    tb = SlotTable(64, len(set(s5.timesteps) | set(s7.timesteps)) - 1)
    tb.add(s5)
    with pytest.raises(RuntimeError, match="time-embedding table is full"):
        tb.add(s7)
    assert len(tb.t) == 5 and len(tb.timesteps) == 5
    server = _server(4, 2)
    with pytest.raises(NotImplementedError, match="'ddim' schedules only"):
        server.submit(schedule=ffhq_ddim_scheduler().stochastic_schedule(5, 0.5))
    with pytest.raises(ValueError, match="latents"):
        server.submit(3, latents=torch.zeros(1, 2, 2, 2))
    assert not server._queue[0]


# ------------------------------------------------------------------------------------------------ 2. utilisation
def test_utilisation_within_grahams_bound_at_one_step_per_graph():
    B = 4
    server = _server(B, 1)
    tickets = _submit_all(server, LENGTHS)
    server.run()
    _check_results(tickets, LENGTHS)
    bound = sum(LENGTHS) / B + (1 - 1 / B) * max(LENGTHS)           # list scheduling: any refill-on-finish order stays within it
    ideal = math.ceil(sum(LENGTHS) / B)
    print(f"[slots host] {len(LENGTHS)} requests, {sum(LENGTHS)} evaluations on {B} slots: {server.replays} replays "
          f"(ideal {ideal}, bound {bound}); useful share {server.useful / server.evaluations:.3f}")
    assert bound == 21.25 and ideal == 18
    assert ideal <= server.replays <= bound, server.replays


# ------------------------------------------------------------------------------------------------ 3. grouping policy
def test_no_group_exceeds_the_smallest_remaining_count_while_requests_wait():
    server = _server(4, 3)
    eng = server.engines[0]
    seen = []

    def before_step(k):
        occupied = [r for r in eng.remaining() if r > 0]
        seen.append((k, min(occupied), max(occupied), len(server._queue[0])))
    eng.before_step = before_step
    tickets = _submit_all(server, LENGTHS)
    server.run()
    _check_results(tickets, LENGTHS)
    assert any(waiting for _, _, _, waiting in seen) and any(not waiting for _, _, _, waiting in seen)
    for k, smallest, largest, waiting in seen:
        assert 1 <= k <= 3
        assert k <= (smallest if waiting else largest), (k, smallest, largest, waiting)
    assert server.group_size([5, 2, 4], True) == 2 and server.group_size([5, 2, 4], False) == 3
    assert server.group_size([1, 2], False) == 2 and server.group_size([7], True) == 3
