"""Counter-based device noise, the host side without a GPU: tests/noise_oracle.py against the Random123 known answers and the
moments of a normal sample, DDIMScheduler.seeded_schedule, SeededSlotTable, the binding of libafldm_noise.so and SamplingServer's
seeded requests against a counting engine (tests/test_slots_host.py)."""
import math
import types

import numpy as np
import pytest
import torch

import noise_oracle as no
from test_slots_host import CountingEngine

N = 1 << 20

# Random123's kat_vectors for philox4x32-10: (counter, key, output)
KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def _ddim():
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    return ffhq_ddim_scheduler()


def moments(z):
    """(mean, var - 1, kurtosis - 3) of a float64 sample."""
    z = np.asarray(z, dtype=np.float64)
    m = z.mean()
    v = ((z - m) ** 2).mean()
    return m, v - 1.0, ((z - m) ** 4).mean() / v ** 2 - 3.0


def check_moments(z, what):
    """The 5 sigma bounds of a normal sample of len(z) values."""
    n = len(z)
    m, v, k = moments(z)
    print(f"[counter noise] {what}: mean {m:.2e} (<= {5 / math.sqrt(n):.2e}), var - 1 {v:.2e} (<= {5 * math.sqrt(2 / n):.2e}), "
          f"kurtosis - 3 {k:.2e} (<= {5 * math.sqrt(24 / n):.2e})")
    assert abs(m) <= 5 / math.sqrt(n) and abs(v) <= 5 * math.sqrt(2 / n) and abs(k) <= 5 * math.sqrt(24 / n), (what, m, v, k)


def check_cross(a, b, what):
    c = float((np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)).mean())
    print(f"[counter noise] cross moment, {what}: {c:.2e} (<= {5 / math.sqrt(len(a)):.2e})")
    assert abs(c) <= 5 / math.sqrt(len(a)), (what, c)


# ------------------------------------------------------------------------------------------------ 1. the stream
def test_known_answers():
    for counter, key, want in KNOWN:
        got = no.philox(np.array([counter], dtype=np.uint32), key)
        assert [int(v) for v in got[0]] == list(want), (counter, key, [hex(int(v)) for v in got[0]])
    # the seed's key and the counter layout: seed = k0 + 2^32 k1, counter (g0 + g, ordinal, slot, c3)
    seed = 0xa4093822 | (0x299f31d0 << 32)
    assert seed < 2 ** 63 and no.key_of(seed) == (0xa4093822, 0x299f31d0)
    got = no.words(seed, 3, g0=0x243f6a88 - 1, ordinal=0x85a308d3, slot=0x13198a2e, c3=0x03707344)
    assert [int(v) for v in got[1]] == list(KNOWN[2][2])


def test_uniforms_and_the_range_of_the_normals():
    lo, hi = ((np.uint32(0) >> 9) + 0.5) * 2.0 ** -23, ((np.uint32(0xffffffff) >> 9) + 0.5) * 2.0 ** -23
    assert lo == 2.0 ** -24 and hi == 1 - 2.0 ** -24
    assert np.float32(lo) == lo and np.float32(hi) == hi                      # exact in fp32
    assert math.sqrt(-2 * math.log(lo)) <= 5.77
    z = no.normals(12345, 3, 4099)
    assert z.shape == (4099,) and np.abs(z).max() <= 5.77
    # element 4 g + k is lane k of group g, whatever the length asked for
    assert np.array_equal(no.normals(12345, 3, 10), z[:10])


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_moments(seed):
    check_moments(no.normals(seed, 3, N), f"seed {seed}, ordinal 3, slot 0, 2^20 values")


def test_cross_moments():
    base = no.normals(7, 0, N)
    check_cross(base, no.normals(7, 1, N), "seed 7, ordinal 0 against 1")
    check_cross(base, no.normals(8, 0, N), "seed 7 against 8")
    check_cross(base, no.normals(7, 0, N, slot=1), "seed 7, slot 0 against 1")
    # a seed above 2^32 differs from its low half
    assert not np.array_equal(no.normals(7 + (1 << 32), 0, 16), base[:16])


def test_update32_is_the_stated_order():
    g = np.random.default_rng(5)
    x, e, z = (g.standard_normal(4096).astype(np.float32) for _ in range(3))
    row = (1.3, -0.7, -0.9, 1.1, 0.4, 0.8, 0.3, 0.6)
    f = np.float32
    p, q, lo, hi, a, b, d, c = (f(v) for v in row)
    t = (p * x).astype(f) + (q * e).astype(f)
    x0 = np.clip(t, lo, hi)
    want = (((a * x).astype(f) + (b * x0).astype(f)).astype(f) + (d * e).astype(f)).astype(f) + (c * z).astype(f)
    got = no.update32(x, e, z, row)
    assert got.dtype == f and np.array_equal(got, want) and (x0 != t).any()
    e[3] = np.nan
    out = no.update32(x, e, z, row)
    assert np.isnan(out[3]) and np.array_equal(np.delete(out, 3), np.delete(got, 3))
    ref = no.update64(torch.from_numpy(x[:3]).double(), torch.from_numpy(e[:3]).double(), torch.from_numpy(z[:3]).double(), row)
    assert np.abs(got[:3] - ref.numpy()).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ 2. the schedule
def test_seeded_schedule_has_the_stochastic_rows_and_no_draws():
    from afldm_amd.schedulers.schedule import KINDS, NOISE_SLOTS, ROW_WIDTH
    assert KINDS["seeded"] == (8, 1, False) and ROW_WIDTH["seeded"] == 8 and "seeded" not in NOISE_SLOTS
    for n, eta in ((6, 0.7), (50, 1.0), (3, 0.0)):
        sde, seeded = _ddim().stochastic_schedule(n, eta), _ddim().seeded_schedule(n, eta)
        assert seeded.kind == "seeded" and sde.kind == "sde"
        assert seeded.rows == sde.rows and seeded.timesteps == sde.timesteps and len(seeded.rows) == n
        assert not any(seeded.draws) and all(sde.draws) and len(seeded.draws) == n
        assert seeded.key != sde.key and seeded.key == _ddim().seeded_schedule(n, eta).key
        assert seeded.init_noise_sigma == sde.init_noise_sigma
        assert [seeded.slots(k) for k in range(n)] == [()] * n
    assert _ddim().seeded_schedule(6, 0.7).key != _ddim().seeded_schedule(6, 0.8).key
    assert all(r[7] == 0.0 for r in _ddim().seeded_schedule(3, 0.0).rows)
    assert all(r[7] > 0.0 for r in _ddim().seeded_schedule(6, 0.7).rows[:-1])


# ------------------------------------------------------------------------------------------------ 3. the table
def _dpm():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, solver_order=2)


def test_seeded_table_codes_and_ordinals():
    from afldm_amd.engine import SeededSlotTable, SlotTable
    assert SlotTable.KIND_CODES == {"ddim": 0, "dpm": 1}
    assert SeededSlotTable.KIND_CODES == {"ddim": 0, "dpm": 1, "seeded": 2}
    tb = SeededSlotTable(64, 48, kinds=("ddim", "dpm", "seeded"))
    d3, s4, p2, s6 = _ddim().schedule(3), _ddim().seeded_schedule(4, 0.5), _dpm().schedule(2), _ddim().seeded_schedule(6, 1.0)
    assert tb.add(d3) == (0, 3) and tb.add(s4) == (3, 7) and tb.add(p2) == (7, 9) and tb.add(s6) == (9, 15)
    assert tb.kind == [0] * 3 + [2] * 4 + [1] * 2 + [2] * 6
    # a row's ordinal is its place in its OWN schedule, whatever was added before
    assert tb.ord == [0, 1, 2] + [0, 1, 2, 3] + [0, 1] + [0, 1, 2, 3, 4, 5]
    assert tb.add(_ddim().seeded_schedule(4, 0.5)) == (3, 7) and len(tb.ord) == len(tb.t) == 15
    assert tb.coef[3:7] == list(s4.rows) and all(len(r) == 8 for r in tb.coef[3:7])
    assert SeededSlotTable(8, 8).kinds == ("ddim", "seeded")
    with pytest.raises(ValueError, match="kinds"):
        SeededSlotTable(8, 8, kinds=("ddim", "sde"))
    with pytest.raises(ValueError, match="kinds"):
        SlotTable(8, 8, kinds=("ddim", "seeded"))


def test_a_refused_schedule_leaves_the_seeded_table_unchanged():
    from afldm_amd.engine import SeededSlotTable
    tb = SeededSlotTable(7, 32)
    tb.add(_ddim().seeded_schedule(5, 0.5))

    def state():
        return (list(tb.coef), list(tb.kind), list(tb.ord), list(tb.t), list(tb.temb), list(tb.timesteps), dict(tb.spans))
    before = state()
    with pytest.raises(RuntimeError, match="row table is full"):
        tb.add(_ddim().seeded_schedule(3, 0.5))
    with pytest.raises(NotImplementedError, match="schedules only"):
        tb.add(_dpm().schedule(2))
    with pytest.raises(NotImplementedError, match="schedules only"):
        tb.add(_ddim().stochastic_schedule(2, 0.5))
    assert state() == before and tb.ord == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ 4. the binding
NAMES = {"afldm_philox_bits", "afldm_counter_noise", "afldm_seeded_step", "afldm_slot_step_seeded"}


def test_the_noise_entry_points_are_declared_built_and_bound():
    import os
    import re
    import subprocess
    import sys
    from afldm_amd import _lib, _noise, build, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "afldm_hip_noise.h")).read()
    declared = set(re.findall(r"^int\s+(afldm_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert declared == NAMES == set(_noise.exports()) == set(_lib.NOISE_ABI.functions)
    nm = subprocess.run(["nm", "-D", "--defined-only", _noise.NOISE_PATH], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if " T afldm_" in l} == declared
    assert not declared & set(_lib.EXPORTS) and not declared & set(_lib.SLOTS_ABI.functions)
    assert "noise.hip" in build.NOISE_SOURCES and build.NOISE_LIB.endswith("libafldm_noise.so")
    assert all(callable(getattr(ops, n)) for n in ("philox_bits", "counter_noise", "seeded_step", "slot_step_seeded"))
    assert len(_noise.lib().afldm_slot_step_seeded.argtypes) == 16 and len(_noise.lib().afldm_seeded_step.argtypes) == 13
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    assert all(n in text for n in NAMES)
    # refusals before any launch: NULL pointers, bad shapes
    lib = _noise.lib()
    assert lib.afldm_philox_bits(None, None, 0, 0, 0, 0, 1, 1, None) == -5
    assert lib.afldm_counter_noise(None, None, None, 0, 1, 1, 1, 1, None) == -5
    assert lib.afldm_seeded_step(None, None, None, None, None, None, 0, 1, 1, 1, 1, 0, None) == -5
    assert lib.afldm_slot_step_seeded(None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 0, None) == -5
    assert lib.afldm_philox_bits(16, 16, 0, 0, 0, 0, 0, 1, None) == -1
    assert lib.afldm_counter_noise(16, 16, 16, 0, 1, 0, 1, 1, None) == -1
    assert lib.afldm_seeded_step(16, 16, 16, 16, 16, 16, 0, 1, 1, 0, 1, 0, None) == -1
    assert lib.afldm_slot_step_seeded(16, 16, 16, 16, 16, 16, 16, 16, 16, 0, 1, 1, 1, 1, 0, None) == -1
    assert b"afldm_slot_step_seeded" in _lib.lib.afldm_last_error()
    code = ("import sys; sys.path.insert(0, %r); import afldm_amd, afldm_amd.ops, afldm_amd.engine, afldm_amd.serving; "
            "import afldm_amd.models.unet_2d; print(any('libafldm_noise' in l for l in open('/proc/self/maps')))" % root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert r.stdout.strip().splitlines()[-1] == "False", r.stdout


# ------------------------------------------------------------------------------------------------ 5. the server
class SeededCountingEngine(CountingEngine):
    """The counting engine with a SeededSlotTable; refills are (latents, begin, end, seed) and the seed of every slot is kept."""

    def __init__(self, B, steps_per_graph, kinds, **kw):
        from afldm_amd.engine import SeededSlotTable
        super().__init__(B, steps_per_graph, **kw)
        self.table = SeededSlotTable(self.table.R, self.table.T, kinds=kinds)
        self.seeds, self.seen = [None] * B, []

    def exchange(self, harvests, refills):
        for b, refill in refills.items():
            assert len(refill) == 4 and isinstance(refill[3], int)
            self.seeds[b] = refill[3]
            self.seen.append((float(refill[0].reshape(-1)[0]), refill[3]))
        return super().exchange(harvests, {b: r[:3] for b, r in refills.items()})


def _pipe():
    unet = types.SimpleNamespace(config=types.SimpleNamespace(in_channels=2, sample_size=1), device=torch.device("cpu"),
                                 dtype=torch.float32)
    return types.SimpleNamespace(unet=unet, scheduler=_ddim())


def _server(slots, steps_per_graph, kinds):
    from afldm_amd.serving import SamplingServer
    return SamplingServer(_pipe(), slots, steps_per_graph, kinds=kinds,
                          engine_factory=lambda i: SeededCountingEngine(slots, steps_per_graph, kinds))


@pytest.mark.parametrize("steps_per_graph", [1, 3])
def test_seeds_travel_with_refills(steps_per_graph):
    server = _server(3, steps_per_graph, ("ddim", "dpm", "seeded"))
    eng = server.engines[0]
    lengths = (3, 5, 2, 4, 6, 1, 2)
    etas = (0.0, 0.5, 1.0, 0.0, 0.7, 0.5, 0.0)
    tickets = [server.submit(n, latents=torch.tensor([1000.0 * i, 0.0]).reshape(1, 2, 1, 1), eta=eta,
                             seed=None if i == 0 else 77 + i, solver="dpm" if i == 3 else None)
               for i, (n, eta) in enumerate(zip(lengths, etas))]
    while server.poll(max_replays=1):
        mirror = [0 if s is None else s[1] for s in server._slot[0]]
        assert mirror == eng.remaining(), (mirror, eng.remaining())
    server.run()
    for i, (ticket, n, eta) in enumerate(zip(tickets, lengths, etas)):
        kind = eng.table.kind[ticket._span[0]]
        assert kind == (2 if eta else 1 if i == 3 else 0), (i, kind)
        assert float(ticket.result()[0, 0]) == 1000.0 * i + n
        assert eng.table.ord[ticket._span[0]:ticket._span[1]] == list(range(n))
    # every refill carried its request's seed (0 for a request without one), in arrival order
    assert eng.seen == [(1000.0 * i, 0 if i == 0 else 77 + i) for i in range(len(lengths))]
    assert server.useful == sum(lengths)


def test_an_eta_needs_a_seed_and_a_seeded_server():
    server = _server(2, 2, ("ddim", "seeded"))
    with pytest.raises(ValueError, match="seed"):
        server.submit(3, eta=0.5)
    with pytest.raises(ValueError, match="seed"):
        server.submit(3, eta=0.5, seed=-1)
    with pytest.raises(ValueError, match="seed"):
        server.submit(3, eta=0.5, seed=2 ** 63)
    with pytest.raises(ValueError, match="seed"):
        server.submit(schedule=_ddim().seeded_schedule(3, 0.5))
    with pytest.raises(ValueError, match="solver"):
        server.submit(3, eta=0.5, seed=1, solver="dpm")
    assert not server._queue[0] and server._count == 0 and not server.engines[0].table.t
    # the start latents of a seeded request are manual_seed(seed)'s, unless latents or a generator is given
    from afldm_amd.utils import randn_tensor
    a = server.submit(2, eta=0.5, seed=5)
    b = server.submit(2, eta=0.5, seed=5, generator=torch.Generator().manual_seed(6))
    c = server.submit(2, seed=5)                                       # (eta = 0 with a seed: a "ddim" request from that seed)
    assert torch.equal(a._start, randn_tensor((1, 2, 1, 1), generator=torch.Generator().manual_seed(5)))
    assert torch.equal(b._start, randn_tensor((1, 2, 1, 1), generator=torch.Generator().manual_seed(6)))
    assert torch.equal(c._start, a._start) and (a.seed, b.seed, c.seed) == (5, 5, 5)
    server.run()
    kinds = [server.engines[0].table.kind[t._span[0]] for t in (a, b, c)]
    assert kinds == [2, 2, 0] and all(t.done() for t in (a, b, c))
    # a server without "seeded": the engine's refusal, and nothing queued
    from afldm_amd.serving import SamplingServer
    from test_slots_dpm_host import KindsCountingEngine
    for kinds in (("ddim",), ("ddim", "dpm")):
        plain = SamplingServer(_pipe(), 2, 2, kinds=kinds, engine_factory=lambda i: KindsCountingEngine(2, 2, kinds))
        with pytest.raises(NotImplementedError, match="schedules only"):
            plain.submit(3, eta=0.5, seed=1)
        assert not plain._queue[0] and plain._count == 0
        t = plain.submit(2, latents=torch.zeros(1, 2, 1, 1))           # and its refills stay (latents, begin, end)
        plain.run()
        assert float(t.result()[0, 0]) == 2
    assert SamplingServer.default_kinds(_pipe()) == ("ddim",)
