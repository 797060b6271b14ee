"""Outpainting (RePaint on a MultiDiffusion canvas), host side (no GPU): the "outpaint" Schedule, the float64 restatement the GPU
tests compare against (tests/outpaint_oracle.py) on its own invariants, the paste and mask helper (afldm_amd.panorama.place) and the
bindings' bookkeeping."""
import math
import os
import subprocess
import sys

import pytest
import torch

import outpaint_oracle as oo
import pano_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


# ------------------------------------------------------------------------------------------------ schedule
def test_outpaint_schedule_is_the_repaint_schedule_under_its_own_kind_and_key():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    from afldm_amd.schedulers.schedule import KINDS, NOISE_SLOTS, ROW_WIDTH
    assert KINDS["outpaint"] == (12, 3, True) and ROW_WIDTH["outpaint"] == 12 and NOISE_SLOTS["outpaint"] == 3
    for cfg in (FFHQ_DDIM_CONFIG, dict(FFHQ_DDIM_CONFIG, set_alpha_to_one=True), dict(FFHQ_DDIM_CONFIG, clip_sample=True)):
        sch = DDIMScheduler.from_config(cfg)
        for n, eta, jl, js in ((6, 0.7, 2, 2), (8, 1.0, 3, 2), (5, 0.0, 10, 10), (4, 0.0, 2, 1)):
            s = sch.outpaint_schedule(n, eta, jl, js)
            assert sch.outpaint_schedule(n, eta, jl, js) is s                                        # made once per key
            r = sch.repaint_schedule(n, eta, jl, js)
            assert s.kind == "outpaint" and r.kind == "repaint"
            assert s.timesteps == r.timesteps and s.rows == r.rows and s.draws == r.draws            # float for float
            assert [s.slots(k) for k in range(len(s.rows))] == [r.slots(k) for k in range(len(r.rows))]
            assert s.init_noise_sigma == r.init_noise_sigma and s.noise_dtype == r.noise_dtype
            assert s.key != r.key
            assert s.key != sch.outpaint_schedule(n + 1, eta, jl, js).key and s.key != sch.outpaint_schedule(n, eta + 0.1, jl, js).key
            assert s.key != sch.outpaint_schedule(n, eta, jl + 1, js).key and s.key != sch.outpaint_schedule(n, eta, jl, js + 1).key
            assert tuple(s.table("cpu").shape) == (len(s.rows), 12)
            last = s.rows[-1]
            assert (last[7], last[8], last[9], last[10]) == (1.0, 0.0, 1.0, 0.0)
    s = DDIMScheduler.from_config(FFHQ_DDIM_CONFIG).outpaint_schedule(6, 0.0, 2, 2)
    assert len(s.rows) > 6 and any(row[10] != 0.0 for row in s.rows)                                 # some evaluations jump back up


def test_outpaint_schedule_refuses_what_repaint_schedule_refuses():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    sch = DDIMScheduler.from_config(FFHQ_DDIM_CONFIG)
    for jl, js in ((0, 2), (2, 0), (-1, 1)):
        with pytest.raises(ValueError):
            sch.repaint_schedule(4, 0.0, jl, js)
        with pytest.raises(ValueError):
            sch.outpaint_schedule(4, 0.0, jl, js)
    v = DDIMScheduler.from_config(dict(FFHQ_DDIM_CONFIG, prediction_type="v_prediction"))
    with pytest.raises(NotImplementedError):
        v.repaint_schedule(4)
    with pytest.raises(NotImplementedError):
        v.outpaint_schedule(4)


# ------------------------------------------------------------------------------------------------ the float64 restatement
ROW = (1.0, -0.9, -1.0, 1.0, 0.55, 0.1, 0.2, 0.8, 0.6, 0.9, 0.43, 0.0)               # clipped, all three slots live
LAST = (1 / 0.6, -0.8 / 0.6, -INF, INF, 0.7, 0.5, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0)      # the last evaluation's shape


def _inputs(P, C, g, seed=0):
    gen = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)
    x, e, known = rn(P, C, g.Hc, g.Wc), rn(P * g.nwin, C, g.S, g.S), rn(P, C, g.Hc, g.Wc)
    zs = [rn(P, C, g.Hc, g.Wc) for _ in range(3)]
    mask = torch.rand(P, 1, g.Hc, g.Wc, generator=gen, dtype=torch.float64)
    wt = torch.rand(g.S, g.S, generator=gen, dtype=torch.float64) + 0.25
    return x, e, known, mask, zs, wt


def test_oracle_single_window_is_the_repaint_formula():
    from afldm_amd.panorama import Geometry
    g = Geometry.grid(5, 5, 5, 5, 5)
    assert g.nwin == 1
    x, e, known, mask, zs, wt = _inputs(2, 3, g)
    for row in (ROW, LAST):
        out, wins, unknown, knownp = oo.outpaint_step(x, e, known, mask, zs, wt, g, row)
        assert float((out - oo.repaint_single(x, e, known, mask, zs, row)).abs().max()) <= 1e-14
        assert torch.equal(wins, out)


@pytest.mark.parametrize("shape", [(4, 11, 4, 3, 3, False), (6, 7, 4, 2, 2, False), (4, 9, 4, 3, 3, True)])
def test_oracle_without_a_mask_is_the_panorama_step_and_with_a_full_one_the_known_content(shape):
    from afldm_amd.panorama import Geometry
    Hc, Wc, S, sy, sx, circ = shape
    g = Geometry.grid(Hc, Wc, S, sy, sx, circular_x=circ)
    x, e, known, mask, zs, wt = _inputs(2, 3, g, seed=1)
    zero, one = torch.zeros_like(mask), torch.ones_like(mask)
    # m = 0, k and u trivial: MultiDiffusion's step on the 8-wide row (p, q, lo, hi, 0, a, b, c) with z_u as its noise
    for row in (ROW, LAST):
        trivial = row[:7] + (1.0, 0.0, 1.0, 0.0, 0.0)
        out, wins, unknown, _ = oo.outpaint_step(x, e, known, zero, zs, wt, g, trivial)
        want, want_wins = po.pano_step(x, e, zs[1], wt, g, row[:4] + (0.0, row[4], row[5], row[6]))
        assert float((out - want).abs().max()) <= 1e-14 and torch.equal(out, unknown)
        assert torch.equal(wins, po.crop(out, g)) and tuple(wins.shape) == (2 * g.nwin, 3, S, S)
    # m = 1 on the last row: the known content, exactly, whatever the model says
    bad = e.clone()
    bad[0] = math.nan
    out, wins, _, knownp = oo.outpaint_step(x, bad, known, one, [None, None, None], wt, g, LAST)
    assert torch.equal(out, known) and torch.equal(knownp, known) and torch.equal(wins, po.crop(known, g))
    # a soft mask is the blend of the two parts
    out, _, unknown, knownp = oo.outpaint_step(x, e, known, mask, zs, wt, g, ROW)
    assert torch.equal(out, ROW[9] * (mask * knownp + (1.0 - mask) * unknown) + ROW[10] * zs[2])
    # a batch-1 mask is broadcast
    out1 = oo.outpaint_step(x, e, known, mask[:1], zs, wt, g, ROW)[0]
    assert torch.equal(out1[0], out[0]) and not torch.equal(out1[1], out[1])


def test_oracle_commutes_with_a_roll_by_the_stride_on_a_circular_axis():
    from afldm_amd.panorama import Geometry
    g = Geometry.grid(4, 9, 4, 3, 3, circular_x=True)
    x, e, known, mask, zs, _ = _inputs(2, 3, g, seed=2)
    ones = torch.ones(4, 4, dtype=torch.float64)
    out = oo.outpaint_step(x, e, known, mask, zs, ones, g, ROW)[0]
    e_rolled = e.reshape(2, g.nwin, 3, 4, 4).roll(1, 1).reshape(-1, 3, 4, 4)

    def r(t):
        return t.roll(3, -1)
    out_r, wins_r = oo.outpaint_step(r(x), e_rolled, r(known), r(mask), [r(z) for z in zs], ones, g, ROW)[:2]
    assert float((out_r - r(out)).abs().max()) <= 1e-14
    assert torch.equal(wins_r, po.crop(out_r, g))


def test_oracle_sampling_loop_draws_where_the_schedule_does():
    from afldm_amd.panorama import Geometry
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    g = Geometry.grid(4, 7, 4, 2, 2)
    gen = torch.Generator().manual_seed(3)
    x, known = torch.randn(1, 2, 4, 7, generator=gen), torch.randn(1, 2, 4, 7, generator=gen)
    mask = torch.zeros(1, 1, 4, 7)
    mask[..., 2:5] = 1.0
    calls = []

    def unet(w, t):
        assert w.dtype == torch.float32 and tuple(w.shape) == (g.nwin, 2, 4, 4)
        return 0.1 * w

    def draw():
        calls.append(1)
        return torch.zeros(1, 2, 4, 7)
    for eta in (0.0, 0.7):
        sched = ffhq_ddim_scheduler().outpaint_schedule(4, eta, 2, 2)
        calls.clear()
        out = oo.sample(unet, x, known, mask, g, sched, draw)
        assert len(calls) == sum(len(sched.slots(k)) for k in range(len(sched.rows))) > 0
        assert tuple(out.shape) == (1, 2, 4, 7) and torch.isfinite(out).all()
        assert torch.equal(out[..., 2:5], known.double()[..., 2:5])                    # kept latents come back exactly


# ------------------------------------------------------------------------------------------------ the paste and the mask
def test_place_centres_wraps_and_shrinks():
    from afldm_amd.panorama import place
    import afldm.panorama as alias
    assert alias.place is place
    p = place(4, 12, 4)
    assert (p.top, p.left, p.rows, p.cols) == (0, 4, (0, 1, 2, 3), (4, 5, 6, 7)) and p.keep_rows == p.rows and p.keep_cols == p.cols
    p = place(8, 11, 4)
    assert (p.top, p.left) == (2, 3)
    p = place(6, 12, 4, top=2, left=8)                                                # flush with the right edge
    assert p.rows == (2, 3, 4, 5) and p.cols == (8, 9, 10, 11)
    p = place(4, 10, 4, left=8, wrap_x=True)                                          # the paste wraps modulo the width
    assert p.cols == (8, 9, 0, 1) and p.rows == (0, 1, 2, 3)
    m = p.mask(4, 10)
    assert len(m) == 4 and all(len(r) == 10 for r in m)
    assert m[0] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]
    p = place(6, 10, 4, top=1, left=8, margin=1, wrap_x=True)
    assert (p.keep_rows, p.keep_cols) == ((2, 3), (9, 0)) and p.rows == (1, 2, 3, 4)
    m = torch.tensor(p.mask(6, 10))
    assert float(m.sum()) == 4.0 and bool((m[2:4][:, [9, 0]] == 1.0).all())
    p = place(5, 9, 5, margin=2)
    assert (p.keep_rows, p.keep_cols) == ((2,), (4,))


def test_place_refuses_positions_off_the_grid_or_outside_the_canvas():
    from afldm_amd.panorama import place
    for kw in (dict(top=0.5), dict(left=2.5), dict(top=-1), dict(top=3), dict(left=-1), dict(left=9), dict(margin=2), dict(margin=-1),
               dict(margin=0.5)):
        with pytest.raises(ValueError):
            place(6, 12, 4, **kw)
    with pytest.raises(ValueError):
        place(6, 12, 4, left=12, wrap_x=True)                                         # a wrapping axis takes corners below its extent
    with pytest.raises(ValueError):
        place(6, 12, 4, top=3, wrap_x=True)                                           # the y axis does not wrap
    with pytest.raises(ValueError):
        place(3, 12, 4)
    assert place(6, 12, 4, left=11, wrap_x=True).cols == (11, 0, 1, 2)
    assert place(6, 12, 4, top=2.0, left=8.0).left == 8                               # integral floats are on the grid


# ------------------------------------------------------------------------------------------------ bindings
def test_outpaint_entry_point_is_bound_and_documented():
    from afldm_amd import _lib, build, ops
    name = "afldm_pano_repaint_step"
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name + "(" in hdr and name in doc
    assert "pano.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "afldm_amd", "csrc", "pano.hip")).read()
    assert 'extern "C" int ' + name + "(" in src
    assert callable(ops.pano_repaint_step)
    # no CPU path
    from afldm_amd.panorama import Geometry
    g = Geometry.grid(4, 7, 4, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pano_repaint_step(torch.zeros(1, 2, 4, 7), torch.zeros(g.nwin, 4, 4, 2), torch.zeros(1, 2, 4, 7), torch.zeros(1, 1, 4, 7),
                              torch.zeros(1, 3, 1, 2, 4, 7), torch.ones(4, 4), g, torch.zeros(12), torch.zeros(1, dtype=torch.int32))


def test_pipeline_surface():
    import inspect
    from afldm_amd.engine import DenoiseEngine, OutpaintEngine, PanoramaEngine
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    import afldm.pipelines.ldm_pipeline as alias
    assert alias.MyLDMPipeline.outpaint is MyLDMPipeline.outpaint
    sig = inspect.signature(MyLDMPipeline.outpaint_latents)
    assert list(sig.parameters)[1:] == ["known_canvas", "canvas_mask", "stride", "circular", "num_inference_steps", "eta", "jump_length",
                                        "jump_n_sample", "generator", "latents", "use_graph"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["stride"], d["circular"], d["num_inference_steps"], d["eta"], d["jump_length"], d["jump_n_sample"], d["use_graph"]) == \
        (None, False, 50, 0.0, 10, 10, True)
    sig = inspect.signature(MyLDMPipeline.outpaint)
    assert list(sig.parameters)[1:7] == ["image", "height", "width", "top", "left", "keep_margin"]
    assert set(list(sig.parameters)[7:]) == {"stride", "circular", "num_inference_steps", "eta", "jump_length", "jump_n_sample", "generator",
                                             "latents", "use_graph", "composite", "output_type", "return_dict"}
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["top"], d["left"], d["keep_margin"], d["composite"], d["output_type"], d["return_dict"]) == (None, None, 0, True, "pil", True)
    for f in (I2SBLDMPipeline.outpaint_latents, I2SBLDMPipeline.outpaint):
        with pytest.raises(NotImplementedError):
            f(object(), torch.zeros(1, 4, 32, 64), torch.zeros(1, 1, 32, 64))
    assert issubclass(OutpaintEngine, PanoramaEngine) and OutpaintEngine.ONE_BRANCH
    assert list(OutpaintEngine.UPDATES) == ["outpaint"]
    assert "outpaint" not in DenoiseEngine.UPDATES and "outpaint" not in PanoramaEngine.UPDATES
    # the panorama and inpaint signatures are as they were
    assert "known_canvas" not in inspect.signature(MyLDMPipeline.panorama_latents).parameters
    assert "height" not in inspect.signature(MyLDMPipeline.inpaint_latents).parameters


def test_script_exists_and_parses_help():
    script = os.path.join(ROOT, "scripts", "outpaint_ffhq.py")
    assert os.path.exists(script)
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--ckpt", "--random-init", "--image", "--height", "--width", "--left", "--top", "--circular"):
        assert flag in r.stdout, flag
