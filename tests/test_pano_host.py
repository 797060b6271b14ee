"""MultiDiffusion panoramas, host side (no GPU): the window geometry (afldm_amd.panorama), the "pano" Schedule, the float64
restatement the GPU tests compare against (tests/pano_oracle.py) on its own invariants, and the bindings' bookkeeping."""
import math
import os

import pytest
import torch

import pano_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("circular", [False, True])
def test_window_origins_cover_every_position_once_per_window(circular):
    from afldm_amd.panorama import MAX_ORIGINS, window_origins
    seen = 0
    for S in (2, 4, 5, 16):
        for extent in range(S, 4 * S + 1):
            for stride in range(1, S + 1):
                count = -(-extent // stride) if circular else -(-(extent - S) // stride) + 1
                if count > MAX_ORIGINS:
                    with pytest.raises(ValueError, match="at most"):
                        window_origins(extent, S, stride, circular)
                    continue
                o = window_origins(extent, S, stride, circular)
                assert isinstance(o, tuple) and all(isinstance(v, int) for v in o) and len(o) == count, (S, extent, stride, o)
                assert o[0] == 0 and list(o) == sorted(set(o))
                covered = set()
                for v in o:
                    cells = [(v + u) % extent if circular else v + u for u in range(S)]
                    assert len(set(cells)) == S                           # no window covers a position twice
                    assert all(0 <= c < extent for c in cells)            # non-circular windows stay inside
                    covered.update(cells)
                assert covered == set(range(extent)), (S, extent, stride, o)
                if circular:
                    assert o == tuple(k * stride for k in range(count))
                else:
                    assert o[-1] == extent - S                            # the last one is flush
                    assert all(b - a == stride for a, b in zip(o[:-2], o[1:-1])) and (len(o) < 2 or 0 < o[-1] - o[-2] <= stride)
                seen += 1
    assert seen > 500
    assert window_origins(16, 16, 3, circular) == ((0,) if not circular else (0, 3, 6, 9, 12, 15))


def test_window_origins_refusals_and_grid():
    from afldm_amd.panorama import Geometry, feather, window_origins
    import afldm.panorama as alias
    assert alias.window_origins is window_origins
    for circular in (False, True):
        for extent, S, stride in ((3, 4, 2), (8, 4, 0), (8, 4, 5), (8, 0, 1), (64, 4, 3), (18, 2, 1)):
            with pytest.raises(ValueError):
                window_origins(extent, S, stride, circular)
    assert window_origins(11, 4, 3) == (0, 3, 6, 7) and window_origins(9, 4, 3, True) == (0, 3, 6)
    assert window_origins(128, 32, 8) == tuple(range(0, 97, 8))           # the 13 windows of a 32 x 128 strip
    g = Geometry.grid(6, 7, 4, 2, 2)
    assert (g.oy, g.ox, g.ny, g.nx, g.nwin, g.wrap_y, g.wrap_x) == ((0, 2), (0, 2, 3), 2, 3, 6, False, False)
    assert g.corners() == [(0, 0), (0, 2), (0, 3), (2, 0), (2, 2), (2, 3)]
    # frozen and hashable: it is part of the engine cache key
    assert g == Geometry.grid(6, 7, 4, 2, 2) and hash(g) == hash(Geometry.grid(6, 7, 4, 2, 2)) and g != Geometry.grid(6, 7, 4, 2, 2, True)
    with pytest.raises(Exception):
        g.S = 5
    s = Geometry.grid(4, 9, 4, 3, 3, circular_x=True).scaled(8)
    assert (s.Hc, s.Wc, s.S, s.oy, s.ox, s.wrap_x) == (32, 72, 32, (0,), (0, 24, 48), True)
    assert feather(5) == [1.0, 2.0, 3.0, 2.0, 1.0] and feather(4) == [1.0, 2.0, 2.0, 1.0] and min(feather(32)) > 0


# ------------------------------------------------------------------------------------------------ schedule
def test_panorama_schedule_rows_draws_and_key():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler, ffhq_ddim_scheduler
    from afldm_amd.schedulers.schedule import NOISE_SLOTS, ROW_WIDTH
    assert ROW_WIDTH["pano"] == 8 and NOISE_SLOTS["pano"] == 1
    n = 8
    for cfg in (FFHQ_DDIM_CONFIG, dict(FFHQ_DDIM_CONFIG, set_alpha_to_one=True)):
        sch = DDIMScheduler.from_config(cfg)
        for eta in (0.0, 0.7):
            s = sch.panorama_schedule(n, eta)
            assert s.kind == "pano" and len(s.timesteps) == len(s.rows) == n and s.timesteps == tuple(sch._timesteps_host)
            assert s.rows == tuple(tuple(float(v) for v in sch.sde_coefficients(t, eta)) for t in s.timesteps)
            assert s.draws == tuple(r[7] != 0.0 for r in s.rows)
            assert [s.slots(k) for k in range(n)] == [(0,) if d else () for d in s.draws]
            if eta == 0.0:
                assert not any(s.draws)
            else:
                assert all(s.draws[:-1]) and s.draws[-1] == (not cfg.get("set_alpha_to_one", False))
            sde = sch.stochastic_schedule(n, eta if eta else 0.5)
            assert s.key != sde.key and s.key != sch.panorama_schedule(n, 0.3).key and s.key != sch.panorama_schedule(n + 1, eta).key
            assert sch.panorama_schedule(n, eta) is s                     # made once per key
            assert tuple(s.table("cpu").shape) == (n, 8)
    with pytest.raises(NotImplementedError):
        DDIMScheduler.from_config(dict(FFHQ_DDIM_CONFIG, clip_sample=True)).panorama_schedule(n, 0.0)
    with pytest.raises(NotImplementedError):
        DDIMScheduler.from_config(dict(FFHQ_DDIM_CONFIG, prediction_type="v_prediction")).panorama_schedule(n, 0.0)
    assert ffhq_ddim_scheduler().panorama_schedule(n, 0.0).init_noise_sigma == 1.0


# ------------------------------------------------------------------------------------------------ the float64 restatement
ROW = (1.0, -0.9, -1.0, 1.0, 0.4, 0.55, 0.1, 0.2)


def _inputs(P, C, g, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, g.Hc, g.Wc, generator=gen, dtype=torch.float64)
    e = torch.randn(P * g.nwin, C, g.S, g.S, generator=gen, dtype=torch.float64)
    z = torch.randn(P, C, g.Hc, g.Wc, generator=gen, dtype=torch.float64)
    wt = torch.rand(g.S, g.S, generator=gen, dtype=torch.float64) + 0.25
    return x, e, z, wt


def test_oracle_single_window_is_the_sde_formula():
    from afldm_amd.panorama import Geometry
    g = Geometry.grid(5, 5, 5, 5, 5)
    assert g.nwin == 1
    x, e, z, wt = _inputs(2, 3, g)
    for row in (ROW, (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.0, 0.7, 0.5, 0.0)):
        out, wins = po.pano_step(x, e, z, wt, g, row)
        assert float((out - po.sde_single(x, e, z, row)).abs().max()) <= 1e-14
        assert torch.equal(wins, out)


@pytest.mark.parametrize("shape", [(4, 11, 4, 3, 3, False), (6, 7, 4, 2, 2, False), (4, 9, 4, 3, 3, True)])
def test_oracle_windows_are_crops_and_fuse_inverts_crop(shape):
    from afldm_amd.panorama import Geometry
    Hc, Wc, S, sy, sx, circ = shape
    g = Geometry.grid(Hc, Wc, S, sy, sx, circular_x=circ)
    x, e, z, wt = _inputs(2, 3, g, seed=1)
    out, wins = po.pano_step(x, e, z, wt, g, ROW)
    assert torch.equal(wins, po.crop(out, g)) and tuple(wins.shape) == (2 * g.nwin, 3, S, S)
    # window k = iy * nx + ix of canvas P sits at batch entry P * nwin + k
    for P in range(2):
        for k, (oy, ox) in enumerate(g.corners()):
            rows = [(oy + u) % Hc for u in range(S)]
            cols = [(ox + v) % Wc for v in range(S)]
            assert torch.equal(wins[P * g.nwin + k], out[P][:, rows][:, :, cols])
    # a weighted mean of equal values is that value
    assert float((po.fuse(po.crop(x, g), wt, g) - x).abs().max()) <= 1e-14
    # if every window predicts the same noise for an element, the update is the plain one there
    shared = po.crop(z, g)
    out2, _ = po.pano_step(x, shared, z, wt, g, ROW)
    assert float((out2 - po.sde_single(x, z, z, ROW)).abs().max()) <= 1e-13


def test_oracle_commutes_with_a_roll_by_the_stride_on_a_circular_axis():
    from afldm_amd.panorama import Geometry
    g = Geometry.grid(4, 9, 4, 3, 3, circular_x=True)
    x, e, z, _ = _inputs(2, 3, g, seed=2)
    ones = torch.ones(4, 4, dtype=torch.float64)
    out, _ = po.pano_step(x, e, z, ones, g, ROW)
    # rolling the canvas by one stride moves every window's content into its right-hand neighbour
    n = g.nwin
    e_rolled = e.reshape(2, n, 3, 4, 4).roll(1, 1).reshape(-1, 3, 4, 4)
    out_r, wins_r = po.pano_step(x.roll(3, -1), e_rolled, z.roll(3, -1), ones, g, ROW)
    assert float((out_r - out.roll(3, -1)).abs().max()) <= 1e-14
    assert torch.equal(wins_r, po.crop(out_r, g))


def test_oracle_sampling_loop_draws_where_the_schedule_does():
    from afldm_amd.panorama import Geometry
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    g = Geometry.grid(4, 7, 4, 2, 2)
    x = torch.randn(1, 2, 4, 7, generator=torch.Generator().manual_seed(3))
    calls = []

    def unet(w, t):
        assert w.dtype == torch.float32 and tuple(w.shape) == (g.nwin, 2, 4, 4)
        return 0.1 * w

    def draw():
        calls.append(1)
        return torch.zeros(1, 2, 4, 7)
    for eta, want in ((0.0, 0), (0.7, 4)):
        calls.clear()
        out = po.sample(unet, x, g, ffhq_ddim_scheduler().panorama_schedule(4, eta), draw)
        assert len(calls) == want and tuple(out.shape) == (1, 2, 4, 7) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ bindings
def test_pano_entry_points_are_bound_and_documented():
    from afldm_amd import _lib, build, ops
    names = ("afldm_pano_step", "afldm_window_fuse", "afldm_window_crop")
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in names:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name + "(" in hdr and name in doc
    assert "pano.hip" in build.SOURCES
    for f in ("pano_step", "window_fuse", "window_crop"):
        assert callable(getattr(ops, f))
    # no CPU path
    from afldm_amd.panorama import Geometry
    g = Geometry.grid(4, 7, 4, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.window_crop(torch.zeros(1, 2, 4, 7), g)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.window_fuse(torch.zeros(g.nwin, 2, 4, 4), torch.ones(4, 4), g)


def test_pipeline_surface():
    import inspect
    from afldm_amd.engine import DenoiseEngine, PanoramaEngine
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    sig = inspect.signature(MyLDMPipeline.panorama_latents)
    assert list(sig.parameters)[1:] == ["height", "width", "stride", "circular", "eta", "num_inference_steps", "batch_size", "generator",
                                        "latents", "use_graph"]
    assert sig.parameters["stride"].default is None and sig.parameters["eta"].default == 0.0
    sig = inspect.signature(MyLDMPipeline.panorama)
    assert (sig.parameters["height"].default, sig.parameters["width"].default, sig.parameters["output_type"].default) == (256, 1024, "pil")
    for f in (I2SBLDMPipeline.panorama_latents, I2SBLDMPipeline.panorama):
        with pytest.raises(NotImplementedError):
            f(object(), 32, 64)
    assert issubclass(PanoramaEngine, DenoiseEngine) and PanoramaEngine.ONE_BRANCH and "pano" not in DenoiseEngine.UPDATES
    assert os.path.exists(os.path.join(ROOT, "scripts", "panorama_ffhq.py"))
