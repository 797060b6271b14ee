"""High-resolution sampling (local + dilated windows, after DemoFusion), host side (no GPU): the "hires" Schedule against its
formulas restated here, the float64 restatement the GPU tests compare against (tests/hires_oracle.py) on its own invariants - the
fractional-shift identity of the low-passed dilated views, the interpolating upsampler, the reductions to the outpainting and
single-window steps - and the bindings' bookkeeping."""
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hires_oracle as ho
import outpaint_oracle as oo
import pano_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


# ------------------------------------------------------------------------------------------------ schedule
def _kappa(t, T):
    return 0.5 * (1.0 + math.cos(math.pi * (T - t) / T))


def _want_rows(sch, n, eta, a1, a2, a3):
    """The rows of the issue's definition, restated: (p..c) = _reverse_row(ab, ab', eta), g = kappa(t_i)^a2, and k0, k1, r, f of the
    NEXT level (1, 0, 0, 0 on the last evaluation)."""
    sch.set_timesteps(n)
    ts = list(sch._timesteps_host)
    T = sch.config.num_train_timesteps
    rows = []
    for i, t in enumerate(ts):
        ab = float(sch.alphas_cumprod[t])
        abn = float(sch.alphas_cumprod[ts[i + 1]]) if i + 1 < n else float(sch.final_alpha_cumprod)
        sigma = eta * math.sqrt((1 - abn) / (1 - ab) * (1 - ab / abn))
        rev = (1 / math.sqrt(ab), -math.sqrt(1 - ab) / math.sqrt(ab), -INF, INF, math.sqrt(abn),
               math.sqrt(max(1 - abn - sigma * sigma, 0.0)), sigma)
        g = 0.0 if a2 is None else _kappa(t, T) ** a2
        if i + 1 < n:
            tn = ts[i + 1]
            tail = (math.sqrt(abn), math.sqrt(1 - abn), 0.0 if a1 is None else _kappa(tn, T) ** a1, g,
                    0.0 if a3 is None else _kappa(tn, T) ** a3)
        else:
            tail = (1.0, 0.0, 0.0, g, 0.0)
        rows.append(rev + tail)
    return ts, rows


@pytest.mark.parametrize("alpha_to_one", [False, True])
def test_hires_schedule_rows_are_the_definition(alpha_to_one):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    from afldm_amd.schedulers.schedule import KINDS, NOISE_SLOTS, ROW_WIDTH
    assert KINDS["hires"] == (12, 1, True) and ROW_WIDTH["hires"] == 12 and NOISE_SLOTS["hires"] == 1
    sch = DDIMScheduler.from_config(dict(FFHQ_DDIM_CONFIG, set_alpha_to_one=alpha_to_one))
    for n, eta, a1, a2, a3 in ((6, 0.0, 3.0, 1.0, 1.0), (5, 0.7, 2.0, 0.5, 1.5), (4, 1.0, None, 1.0, None), (7, 0.0, 3.0, None, 1.0),
                               (1, 0.7, 3.0, 1.0, 1.0)):
        s = sch.hires_schedule(n, eta, a1, a2, a3)
        assert sch.hires_schedule(n, eta, a1, a2, a3) is s                                             # made once per key
        ts, rows = _want_rows(sch, n, eta, a1, a2, a3)
        assert s.kind == "hires" and list(s.timesteps) == ts and len(s.rows) == n
        for got, want in zip(s.rows, rows):
            assert len(got) == 12
            for a, b in zip(got, want):
                assert a == b or abs(a - b) <= 1e-15 * max(1.0, abs(b)), (got, want)
        last = s.rows[-1]
        assert last[7:10] == (1.0, 0.0, 0.0) and last[11] == 0.0 and last[10] == rows[-1][10]          # (..., 1, 0, 0, g, 0)
        # a step draws exactly where c != 0
        assert list(s.draws) == [r[6] != 0.0 for r in s.rows]
        assert [s.slots(k) for k in range(n)] == [((0,) if r[6] != 0.0 else ()) for r in s.rows]
        if eta == 0.0:
            assert not any(s.draws)
        elif n > 1:
            assert any(s.draws)
        assert tuple(s.table("cpu").shape) == (n, 12)
        # None switches a term off in every row
        assert (a1 is not None) or all(r[9] == 0.0 for r in s.rows)
        assert (a2 is not None) or all(r[10] == 0.0 for r in s.rows)
        assert (a3 is not None) or all(r[11] == 0.0 for r in s.rows)
        if n > 1:
            assert (a1 is None) or all(0.0 < r[9] <= 1.0 for r in s.rows[:-1])
            assert (a2 is None) or all(0.0 < r[10] <= 1.0 for r in s.rows)
            assert (a3 is None) or all(0.0 < r[11] <= 1.0 for r in s.rows[:-1])
        # the start: the first level, and the first input's low-pass
        k0, k1, f0 = sch.hires_start(n, a3)
        ab0 = float(sch.alphas_cumprod[ts[0]])
        assert (k0, k1) == (math.sqrt(ab0), math.sqrt(1 - ab0))
        assert f0 == (0.0 if a3 is None else _kappa(ts[0], sch.config.num_train_timesteps) ** a3)


def test_hires_schedule_keys_and_refusals():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    sch = DDIMScheduler.from_config(FFHQ_DDIM_CONFIG)
    base = (6, 0.5, 3.0, 1.0, 1.0)
    s = sch.hires_schedule(*base)
    others = [(7, 0.5, 3.0, 1.0, 1.0), (6, 0.6, 3.0, 1.0, 1.0), (6, 0.5, 2.0, 1.0, 1.0), (6, 0.5, 3.0, 2.0, 1.0), (6, 0.5, 3.0, 1.0, 2.0),
              (6, 0.5, None, 1.0, 1.0), (6, 0.5, 3.0, None, 1.0), (6, 0.5, 3.0, 1.0, None)]
    keys = {sch.hires_schedule(*o).key for o in others}
    assert len(keys) == len(others) and s.key not in keys
    assert s.key != sch.panorama_schedule(6, 0.5).key and s.key != sch.stochastic_schedule(6, 0.5).key
    assert s.key != sch.outpaint_schedule(6, 0.5).key and s.key != sch.ilvr_schedule(6, 0.5).key
    # the defaults
    d = {k: v.default for k, v in inspect.signature(DDIMScheduler.hires_schedule).parameters.items()}
    assert (d["eta"], d["cosine_scale_1"], d["cosine_scale_2"], d["cosine_scale_3"]) == (0.0, 3.0, 1.0, 1.0)
    assert sch.hires_schedule(6).rows == sch.hires_schedule(6, 0.0, 3.0, 1.0, 1.0).rows
    # the same refusals as panorama_schedule
    for bad in (dict(clip_sample=True), dict(prediction_type="v_prediction")):
        v = DDIMScheduler.from_config(dict(FFHQ_DDIM_CONFIG, **bad))
        with pytest.raises(NotImplementedError):
            v.panorama_schedule(4)
        with pytest.raises(NotImplementedError):
            v.hires_schedule(4)


# ------------------------------------------------------------------------------------------------ the float64 restatement
def _fourier_shift(v, dy, dx):
    """The plane v [S, S] shifted by (dy, dx) samples, fractions included: bin (ky, kx) times exp(2 pi i (ky dy + kx dx) / S), with
    signed frequencies."""
    S = v.shape[-1]
    k = np.fft.fftfreq(S) * S
    ph = np.exp(2j * np.pi * (k[:, None] * dy + k[None, :] * dx) / S)
    return np.fft.ifft2(np.fft.fft2(v) * ph).real


@pytest.mark.parametrize("S,s", [(16, 2), (16, 4), (8, 2), (6, 2)])
def test_lowpassed_dilated_views_are_fractional_shifts_of_one_another(S, s):
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    N = S * s
    L = ilvr_filter(N, s)
    assert L.dtype == torch.float64 and tuple(L.shape) == (N, N)
    x = torch.randn(1, 1, N, N, generator=torch.Generator().manual_seed(S + s), dtype=torch.float64)
    v = ho.views(ho.lowpass(x, L), s)[0, :, 0].numpy()                     # [s^2, S, S]
    worst = 0.0
    for i in range(s):
        for j in range(s):
            worst = max(worst, float(np.abs(v[i * s + j] - _fourier_shift(v[0], i / s, j / s)).max()))
    print(f"[S = {S}, scale {s}] dilated views against the Fourier shifts of view (0, 0): {worst:.2e}")
    assert worst <= 1e-12
    # the unfiltered views are not: the identity is the filter's doing
    u = ho.views(x, s)[0, :, 0].numpy()
    assert float(np.abs(u[1] - _fourier_shift(u[0], 0.0, 1 / s)).max()) > 1e-2
    # ... and the filter keeps 2 (S / 2) - 1 bins per axis, strictly below the decimated Nyquist
    spectrum = np.abs(np.fft.fft(L.numpy()[:, 0]))
    kept = np.nonzero(spectrum > 1e-9)[0]
    assert len(kept) == 2 * (S // 2) - 1 and all(min(k, N - k) < S / 2 for k in kept)


@pytest.mark.parametrize("S,s", [(16, 2), (16, 4), (8, 2), (6, 2), (5, 3), (32, 2)])
def test_the_upsampler_interpolates(S, s):
    from afldm_amd import _lib
    from oracle.ideal_filters import up_matrix
    U = torch.from_numpy(up_matrix(S, s))
    assert tuple(U.shape) == (s * S, S) and U.dtype == torch.float64
    z = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(S), dtype=torch.float64)
    up = ho.upsample(z, U)
    assert tuple(up.shape) == (2, 3, s * S, s * S)
    assert torch.equal(up[..., ::s, ::s], z)                                 # exactly: rows s u of U are unit vectors
    # the library's fp32 matrix (what the pipeline upsamples with) is that matrix rounded, its zeros to 1e-14
    Uf = _lib.filter_matrix(0, S, s)
    assert Uf.dtype == torch.float32 and float((Uf.double() - U).abs().max()) <= 1e-7
    assert float((ho.upsample(z, Uf)[..., ::s, ::s] - z).abs().max()) <= 1e-12


def _inputs(P, C, g, scale, seed=0):
    gen = torch.Generator().manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)
    NW = g.nwin + scale * scale
    x, e = rn(P, C, g.Hc, g.Wc), rn(P * NW, C, g.S, g.S)
    ref, eps_ref, z = rn(P, C, g.Hc, g.Wc), rn(P, C, g.Hc, g.Wc), rn(P, C, g.Hc, g.Wc)
    wt = torch.rand(g.S, g.S, generator=gen, dtype=torch.float64) + 0.25
    return x, e, ref, eps_ref, z, wt


ROW = (1.0, -0.9, -1.0, 1.0, 0.55, 0.1, 0.2, 0.8, 0.6, 0.3, 0.4, 0.7)               # clipped, every term on


@pytest.mark.parametrize("S,s,stride", [(4, 2, 2), (5, 3, 2), (8, 2, 4)])
def test_oracle_without_the_global_terms_is_the_outpaint_step_with_nothing_kept(S, s, stride):
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    from afldm_amd.panorama import Geometry
    g = Geometry.grid(S * s, S * s, S, stride, stride)
    L = ilvr_filter(S * s, s)
    P, C = 2, 3
    x, e, ref, eps_ref, z, wt = _inputs(P, C, g, s, seed=1)
    for c in (0.2, 0.0):
        row = ROW[:6] + (c,) + ROW[7:9] + (0.0, 0.0, 0.7)                    # g = 0, r = 0; f stays: it touches the dilated input only
        out, wins = ho.hires_step(x, e, ref, eps_ref, z, wt, L, g, s, row)
        loc, _ = ho.split(e, g, s)
        rp = row[:7] + (row[7], row[8], 1.0, 0.0, 0.0)                       # the "repaint" row with u0 = 1, u1 = 0
        want, want_wins, _, _ = oo.outpaint_step(x, loc, ref, torch.zeros(P, 1, S * s, S * s, dtype=torch.float64),
                                                 [eps_ref, z, None], wt, g, rp)
        assert float((out - want).abs().max()) <= 1e-14
        got_loc, got_dil = ho.split(wins, g, s)
        assert torch.equal(got_loc, po.crop(out, g)) and float((got_loc - want_wins).abs().max()) <= 1e-14
        y = out + 0.7 * (ho.lowpass(out, L) - out)
        assert torch.equal(got_dil, ho.views(y, s))
        # what the row switches off is not looked at
        nan = torch.full_like(x, math.nan)
        bad = e.clone().reshape(P, -1, C, S, S)
        bad[:, g.nwin:] = math.nan
        out2, _ = ho.hires_step(x, bad.reshape(e.shape), nan, nan, nan if c == 0.0 else z, wt, L, g, s, row)
        assert torch.equal(out2, out)
    # f = 0: plain sub-lattices, and the filter is not looked at
    out, wins = ho.hires_step(x, e, ref, eps_ref, z, wt, torch.full_like(L, math.nan), g, s, ROW[:11] + (0.0,))
    assert torch.equal(ho.split(wins, g, s)[1], ho.views(out, s)) and torch.isfinite(out).all()
    # every term on: the definition, statement by statement
    p, q, lo, hi, a, b, c, k0, k1, r, gm, f = ROW
    out, wins = ho.hires_step(x, e, ref, eps_ref, z, wt, L, g, s, ROW)
    loc, dil = ho.split(e, g, s)
    eg = ho.unviews(dil, s)
    x0m = (1 - gm) * po.fuse(po.x0_windows(x, loc, g, ROW), wt, g) + gm * torch.clamp(p * x + q * eg, lo, hi)
    em = (1 - gm) * po.fuse(loc, wt, g) + gm * eg
    want = r * (k0 * ref + k1 * eps_ref) + (1 - r) * (a * x0m + b * em + c * z)
    assert float((out - want).abs().max()) <= 1e-14
    for i in range(s):
        for j in range(s):
            assert torch.equal(eg[:, :, i::s, j::s], dil[:, i * s + j])      # window nwin + i s + j covers (i + s u, j + s v)


def test_oracle_at_scale_one_the_local_mean_is_the_dilated_prediction():
    """scale = 1: one local window and one dilated window, both the whole canvas.  Given the same eps they predict the same, so
    the mix does not depend on g."""
    from afldm_amd.panorama import Geometry
    S = 6
    g = Geometry.grid(S, S, S, S, S)
    assert g.nwin == 1
    x, e, ref, eps_ref, z, _ = _inputs(2, 3, g, 1, seed=2)
    e = e.reshape(2, 2, 3, S, S)
    e[:, 1] = e[:, 0]
    e = e.reshape(4, 3, S, S)
    ones, eye = torch.ones(S, S, dtype=torch.float64), torch.eye(S, dtype=torch.float64)
    outs = [ho.hires_step(x, e, ref, eps_ref, z, ones, eye, g, 1, ROW[:10] + (gm, 0.0))[0] for gm in (0.0, 0.4, 1.0)]
    assert float((outs[1] - outs[0]).abs().max()) <= 1e-14 and float((outs[2] - outs[0]).abs().max()) <= 1e-14
    wins = ho.hires_windows(x, eye, 0.5, g, 1)
    assert torch.equal(wins.reshape(2, 2, 3, S, S)[:, 0], x) and float((wins.reshape(2, 2, 3, S, S)[:, 1] - x).abs().max()) <= 1e-15


def test_oracle_sampling_loop_draws_where_the_schedule_does():
    from afldm_amd import _lib
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    from afldm_amd.panorama import Geometry
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    S, s = 4, 2
    g = Geometry.grid(8, 8, S, 2, 2)
    NW = g.nwin + 4
    gen = torch.Generator().manual_seed(3)
    base, eps_ref = torch.randn(1, 2, S, S, generator=gen), torch.randn(1, 2, 8, 8, generator=gen)
    U, L = _lib.filter_matrix(0, S, s), ilvr_filter(8, s)
    calls = []

    def unet(w, t):
        assert w.dtype == torch.float32 and tuple(w.shape) == (NW, 2, S, S)
        return 0.1 * w

    def draw():
        calls.append(1)
        return torch.zeros(1, 2, 8, 8)
    for eta in (0.0, 0.7):
        sch = ffhq_ddim_scheduler()
        sched = sch.hires_schedule(4, eta)
        calls.clear()
        out = ho.sample(unet, base, U, L, g, s, sched, sch.hires_start(4, 1.0), eps_ref, draw)
        assert len(calls) == sum(len(sched.slots(k)) for k in range(4)) and (len(calls) > 0) == (eta != 0.0)
        assert tuple(out.shape) == (1, 2, 8, 8) and out.dtype == torch.float64 and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ bindings
def test_hires_entry_points_are_bound_and_documented():
    from afldm_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(ROOT, "afldm_amd", "csrc", "hires.hip")).read()
    for name in ("afldm_hires_step", "afldm_hires_windows"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name + "(" in hdr and name in doc
        assert 'extern "C" int ' + name + "(" in src
    assert "hires.hip" in build.SOURCES
    assert callable(ops.hires_step) and callable(ops.hires_windows)
    # no CPU path
    from afldm_amd.panorama import Geometry
    g = Geometry.grid(8, 8, 4, 2, 2)
    canvas, L = torch.zeros(1, 2, 8, 8), torch.eye(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.hires_step(canvas, torch.zeros(g.nwin + 4, 4, 4, 2), canvas, canvas, None, torch.ones(4, 4), L, L, g, 2, torch.zeros(12),
                       torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.hires_windows(canvas, L, L, 0.5, g, 2)


def test_pipeline_surface():
    from afldm_amd.engine import DenoiseEngine, HiresEngine, OutpaintEngine, PanoramaEngine
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    import afldm.pipelines.ldm_pipeline as alias
    assert alias.MyLDMPipeline.hires is MyLDMPipeline.hires
    sig = inspect.signature(MyLDMPipeline.hires_latents)
    assert list(sig.parameters)[1:] == ["base_latents", "scale", "stride", "eta", "num_inference_steps", "cosine_scale_1",
                                        "cosine_scale_2", "cosine_scale_3", "generator", "use_graph"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["scale"], d["stride"], d["eta"], d["num_inference_steps"], d["cosine_scale_1"], d["cosine_scale_2"], d["cosine_scale_3"],
            d["generator"], d["use_graph"]) == (2, None, 0.0, 50, 3.0, 1.0, 1.0, None, True)
    sig = inspect.signature(MyLDMPipeline.hires)
    assert list(sig.parameters)[1:4] == ["batch_size", "scale", "base_latents"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["batch_size"], d["scale"], d["base_latents"], d["output_type"]) == (1, 2, None, "pil")
    for f in (I2SBLDMPipeline.hires_latents, I2SBLDMPipeline.hires):
        with pytest.raises(NotImplementedError):
            f(object(), torch.zeros(1, 4, 32, 32))
    assert issubclass(HiresEngine, PanoramaEngine) and HiresEngine.ONE_BRANCH
    assert list(HiresEngine.UPDATES) == ["hires"]
    for other in (DenoiseEngine, PanoramaEngine, OutpaintEngine):
        assert "hires" not in other.UPDATES


def test_script_exists_and_parses_help():
    script = os.path.join(ROOT, "scripts", "hires_ffhq.py")
    assert os.path.exists(script)
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--ckpt", "--random-init", "--scale", "--stride", "--steps", "--timings"):
        assert flag in r.stdout, flag
