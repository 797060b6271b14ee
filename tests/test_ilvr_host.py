"""ILVR reference-guided sampling, host side (no GPU): DDIMScheduler.ilvr_schedule - every coefficient row against a float64
restatement from alphas_cumprod, the conditioning range, the draw pattern and the key - the "sde" and "repaint" schedules it must
leave alone, the low-pass matrix (a symmetric projection that is the reference's rfft2 -> mask -> irfft2 and commutes with every
circular shift), argument validation of the pipeline entries, the header, and the ops' refusal of CPU tensors."""
import itertools
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sched(**kw):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    return DDIMScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)


def want_rows(s, n, eta, range_t, bound=math.inf):
    """The rows of the definition in float64, from the scheduler's fp32 alphas_cumprod."""
    s.set_timesteps(n)
    g = [int(t) for t in s.timesteps]
    ac = s.alphas_cumprod.double()
    rows = []
    for i, t in enumerate(g):
        a = float(ac[t])
        ap = float(ac[g[i + 1]]) if i + 1 < n else float(s.final_alpha_cumprod)
        sigma = eta * math.sqrt((1 - ap) / (1 - a) * (1 - a / ap))
        k0, k1 = (math.sqrt(ap), math.sqrt(1 - ap)) if i + 1 < n else (1.0, 0.0)
        rows.append([1 / math.sqrt(a), -math.sqrt(1 - a) / math.sqrt(a), -bound, bound, math.sqrt(ap),
                     math.sqrt(max(1 - ap - sigma ** 2, 0.0)), sigma, k0, k1, 1.0 if t > range_t else 0.0, 0.0, 0.0])
    return g, rows


@pytest.mark.parametrize("n,eta,range_t", list(itertools.product((5, 50), (0.0, 0.7, 1.0), (0, 300, 1000))))
@pytest.mark.parametrize("one", [False, True])
@pytest.mark.parametrize("spacing", ["leading", "trailing", "linspace"])
@pytest.mark.parametrize("clip", [False, True])
def test_rows_and_draws(n, eta, range_t, one, spacing, clip):
    from afldm_amd.schedulers.schedule import NOISE_SLOTS, ROW_WIDTH
    kw = dict(set_alpha_to_one=one, timestep_spacing=spacing, clip_sample=clip)
    il = sched(**kw).ilvr_schedule(n, eta=eta, range_t=range_t)
    g, want = want_rows(sched(**kw), n, eta, range_t, 1.0 if clip else math.inf)
    assert ROW_WIDTH["ilvr"] == 12 and NOISE_SLOTS["ilvr"] == 2
    assert il.kind == "ilvr" and il.noise_dtype is None and il.init_noise_sigma == 1.0
    assert list(il.timesteps) == g and g == sorted(g, reverse=True) and len(set(g)) == n
    assert len(il.rows) == len(il.draws) == n and all(len(r) == 12 for r in il.rows)
    got = il.table("cpu")
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 12)
    assert torch.equal(got, torch.tensor(want, dtype=torch.float64).float())        # to fp32 rounding: the same fp32 numbers
    torch.testing.assert_close(torch.tensor(il.rows, dtype=torch.float64), torch.tensor(want, dtype=torch.float64),
                               rtol=1e-12, atol=1e-15)
    for i, (t, row, d) in enumerate(zip(g, il.rows, il.draws)):
        p, q, lo, hi, a, b, c, k0, k1, w, pad0, pad1 = row
        assert w == (1.0 if t > range_t else 0.0) and (pad0, pad1) == (0.0, 0.0)
        assert (lo, hi) == ((-1.0, 1.0) if clip else (-math.inf, math.inf))
        assert abs(a * a + b * b + c * c - 1) < 1e-12                               # the reverse step keeps the level a_prev
        assert i == n - 1 or abs(k0 * k0 + k1 * k1 - 1) < 1e-12
        assert d == (w != 0.0 and k1 != 0.0, c != 0.0) and il.slots(i) == tuple(j for j in range(2) if d[j])
        if eta == 0.0:
            assert c == 0.0 and not d[1]
    assert il.rows[-1][7:9] == (1.0, 0.0) and not il.draws[-1][0]
    if spacing != "linspace":          # (linspace ends on timestep 0, whose level is final_alpha_cumprod unless that is 1: sigma = 0)
        assert il.draws[-1] == (False, bool(eta) and not one)
    if range_t == 1000:
        assert not any(d[0] for d in il.draws) and all(r[9] == 0.0 for r in il.rows)
    if range_t == 0:
        assert all(r[9] == (1.0 if t > 0 else 0.0) for t, r in zip(g, il.rows))
    if eta and spacing != "linspace":
        assert [d[1] for d in il.draws] == [i < n - 1 or not one for i in range(n)]  # sigma = 0 at a_prev = 1 (set_alpha_to_one)


def test_other_settings():
    il = sched(clip_sample=True, clip_sample_range=2.5).ilvr_schedule(6, 0.3, 100)
    _, want = want_rows(sched(clip_sample=True, clip_sample_range=2.5), 6, 0.3, 100, 2.5)
    assert torch.equal(il.table("cpu"), torch.tensor(want, dtype=torch.float64).float())
    il = sched(clip_sample=False, clip_sample_range=2.5).ilvr_schedule(6, 0.3, 100)
    _, want = want_rows(sched(), 6, 0.3, 100)
    assert torch.equal(il.table("cpu"), torch.tensor(want, dtype=torch.float64).float())
    d = sched().ilvr_schedule(50)                                                   # defaults: eta = 1 (DDPM's ancestral step), range_t = 0
    assert d.config._ilvr_eta == 1.0 and d.config._ilvr_range_t == 0 and d.config._ilvr_steps == 50
    assert all(r[9] == 1.0 for r in d.rows) and d.draws[:-1] == ((True, True),) * 49 and d.draws[-1] == (False, True)
    with pytest.raises(NotImplementedError):
        sched(prediction_type="v_prediction").ilvr_schedule(6)


def test_keys():
    base = dict(num_inference_steps=6, eta=0.5, range_t=200)
    a = sched().ilvr_schedule(**base)
    assert sched().ilvr_schedule(**base) is a                                       # equal settings: the same schedule
    keys = {a.key}
    for k, v in [("num_inference_steps", 8), ("eta", 0.25), ("range_t", 400)]:
        other = sched().ilvr_schedule(**dict(base, **{k: v}))
        assert other.key not in keys, k
        keys.add(other.key)
    assert sched(clip_sample=True).ilvr_schedule(**base).key not in keys
    settings = dict(a.key[1])
    assert a.key[0] == "DDIMScheduler" and settings["_ilvr_steps"] == "6" and settings["_ilvr_eta"] == "0.5"
    assert settings["_ilvr_range_t"] == "200"


def test_other_schedules_are_unaffected():
    from afldm_amd.schedulers import schedule

    def made():
        return sched().stochastic_schedule(7, 0.4), sched().repaint_schedule(6, 0.4, 2, 2), sched().schedule(5)
    before = made()
    sched().ilvr_schedule(6, 0.4, 100)
    schedule._MADE.clear()                                                          # made again, not looked up
    sched().ilvr_schedule(6, 0.4, 100)
    after = made()
    for b, a in zip(before, after):
        assert a is not b and a.key == b.key and a.draws == b.draws and a.rows == b.rows and a.kind == b.kind
        assert not any(k.startswith("_ilvr") for k, _ in a.key[1])
    assert [a.kind for a in after] == ["sde", "repaint", "ddim"]
    assert all(isinstance(d, bool) for d in after[0].draws) and all(isinstance(d, tuple) and len(d) == 3 for d in after[1].draws)
    assert schedule.ROW_WIDTH["sde"] == 8 and schedule.ROW_WIDTH["repaint"] == 12 and schedule.NOISE_SLOTS["repaint"] == 3
    assert schedule.NOISE_SLOTS["sde"] == 1
    with pytest.raises(AssertionError):                                             # two slots: a pair per step, not a bool or a triple
        schedule.Schedule.of(sched(), "ilvr", [1], [(0.0,) * 12], [(True, True, False)], _test_only=2)


# ------------------------------------------------------------------------------------------------ the filter
@pytest.mark.parametrize("S,factor", [(16, 2), (16, 4), (32, 2), (32, 4), (32, 8), (5, 2)])
def test_filter_is_a_shift_equivariant_projection(S, factor):
    from afldm_amd.af_libs.ideal_lpf import _rect_1d, ilvr_filter
    L = ilvr_filter(S, factor)
    assert L.dtype == torch.float64 and tuple(L.shape) == (S, S)
    assert float((L - L.T).abs().max()) <= 1e-14 and float((L @ L - L).abs().max()) <= 1e-14
    r = _rect_1d(S, 1.0 / factor, 0.0).double()
    kept = int(r.sum())
    assert abs(float(torch.trace(L)) - kept) <= 1e-12                               # a projection's trace is its rank
    if S == 32:
        assert kept == {2: 15, 4: 7, 8: 3}[factor]
    g = torch.Generator().manual_seed(S + factor)
    x = torch.randn(3, S, S, generator=g, dtype=torch.float64)
    # the reference's forward: rfft2 -> the separable mask -> irfft2
    mask = (r[:, None] * r[None, :])[:, : S // 2 + 1]
    want = torch.fft.irfft2(torch.fft.rfft2(x) * mask, s=(S, S))
    got = L @ x @ L.T
    assert float((got - want).abs().max()) <= 1e-12
    # an integer roll: the same matrix entries in another place - exact
    assert torch.equal(torch.roll(L, (3, 3), (0, 1)), L)
    rolled = L @ torch.roll(x, (3, 5), (-2, -1)) @ L.T
    assert float((rolled - torch.roll(got, (3, 5), (-2, -1))).abs().max()) <= 1e-13
    # a fractional shift, as a phase ramp in the Fourier domain (odd S: exact; even S: the Nyquist bin, which phi removes
    # anyway, is left out)

    def shift(t, dy, dx):
        f = torch.fft.fftfreq(S, dtype=torch.float64)
        nyq = torch.ones(S, dtype=torch.float64)
        if S % 2 == 0:
            nyq[S // 2] = 0.0
        ph = torch.exp(-2j * math.pi * (f[:, None] * dy + f[None, :] * dx)) * nyq[:, None] * nyq[None, :]
        return torch.fft.ifft2(torch.fft.fft2(t) * ph).real
    a, b = L @ shift(x, 0.3, -1.7) @ L.T, shift(got, 0.3, -1.7)
    assert float((a - b).abs().max()) <= 1e-12


def test_filter_refuses_a_factor_with_no_band():
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    for S, factor in ((32, 32), (16, 16), (16, 0), (16, -2)):
        with pytest.raises(ValueError, match="valid integer factors: 1, 2"):
            ilvr_filter(S, factor)
    assert abs(float(torch.trace(ilvr_filter(32, 16))) - 1) <= 1e-12               # only the mean is left


# ------------------------------------------------------------------------------------------------ pipeline
class _FakeUnet:
    dtype, device = torch.float32, torch.device("cpu")

    class config:
        in_channels, sample_size = 4, 8


class _FakeVae:
    dtype = torch.float32

    class config:
        block_out_channels, scaling_factor = (8, 8, 8), 0.5


def _pipe(scheduler=None, vae=None):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    pipe = MyLDMPipeline(vae, _FakeUnet(), scheduler or sched())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def test_ilvr_latents_routes_to_an_ilvr_engine_in_its_own_slot(monkeypatch):
    from afldm_amd import engine
    from afldm_amd.af_libs.ideal_lpf import ilvr_filter
    seen = []

    class Engine:
        def __init__(self, unet, schedule, batch, steps, use_graph):
            self.schedule = schedule
            seen.append(("init", schedule.kind, batch, steps, use_graph))

        def run(self, latents, draw=None, known=None):
            seen.append(("run", tuple(known[0].shape), known[1]))
            for k in range(len(self.schedule.draws)):
                for _ in self.schedule.slots(k):
                    draw()
            return latents
    monkeypatch.setattr(engine, "DenoiseEngine", Engine)
    pipe = _pipe()
    ref = torch.zeros(2, 4, 8, 8)
    g = torch.Generator().manual_seed(5)
    out = pipe.ilvr_latents(ref, down_factor=2, num_inference_steps=6, generator=g)
    assert tuple(out.shape) == (2, 4, 8, 8)
    assert seen[0] == ("init", "ilvr", 2, 6, True) and seen[1][:2] == ("run", (2, 4, 8, 8))
    L = seen[1][2]
    assert L.dtype == torch.float32 and torch.equal(L, ilvr_filter(8, 2).float())
    assert "_engines" not in pipe.__dict__ and "_repaint_engines" not in pipe.__dict__ and len(pipe._ilvr_engines) == 1
    # the start latents, then per evaluation z_k, z_u where the schedule draws them: all from the caller's generator
    il = sched().ilvr_schedule(6, 1.0, 0)
    want = torch.Generator().manual_seed(5)
    for _ in range(1 + sum(len(il.slots(k)) for k in range(6))):
        torch.randn(2, 4, 8, 8, generator=want)
    assert torch.equal(g.get_state(), want.get_state())
    # another factor or a matrix of the caller's: the cached engine; another range: another one
    pipe.ilvr_latents(ref, down_factor=4, num_inference_steps=6, latents=torch.zeros(2, 4, 8, 8))
    mine = torch.eye(8)
    pipe.ilvr_latents(ref, phi=mine, num_inference_steps=6)
    assert torch.equal(seen[-1][2], mine)
    pipe.ilvr_latents(ref, range_t=500, num_inference_steps=6)
    assert [s[:4] for s in seen if s[0] == "init"] == [("init", "ilvr", 2, 6), ("init", "ilvr", 2, 6)]


def test_argument_validation(monkeypatch):
    from afldm_amd import engine
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    monkeypatch.setattr(engine, "DenoiseEngine", lambda *a, **k: pytest.fail("no engine before the arguments are checked"))
    ref = torch.zeros(2, 4, 8, 8)
    pipe = _pipe()
    for bad, kw in [(torch.zeros(2, 3, 8, 8), {}), (torch.zeros(2, 4, 8, 4), {}), (torch.zeros(4, 8, 8), {}),
                    (ref, dict(latents=torch.zeros(1, 4, 8, 8))), (ref, dict(phi=torch.eye(4))), (ref, dict(phi=torch.zeros(8, 4)))]:
        with pytest.raises(ValueError):
            pipe.ilvr_latents(bad, num_inference_steps=4, **kw)
    with pytest.raises(ValueError, match="valid integer factors: 1, 2, 3, 4$"):       # 8 x 8 plane: 8 leaves no band
        pipe.ilvr_latents(ref, down_factor=8, num_inference_steps=4)
    # no VAE: ilvr refuses, as _deliver does
    with pytest.raises(NotImplementedError, match="VAE"):
        pipe.ilvr(torch.zeros(2, 3, 32, 32))
    # with one: the shape is checked before anything touches the GPU (the fake VAE cannot encode)
    vp = _pipe(vae=_FakeVae())
    for img in (torch.zeros(2, 3, 32, 16), torch.zeros(2, 1, 32, 32), torch.zeros(3, 32, 32)):
        with pytest.raises(ValueError):
            vp.ilvr(img)
    # DPM-Solver: refused by name from both entries
    dp = _pipe(DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG), vae=_FakeVae())
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        dp.ilvr_latents(ref)
    with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
        dp.ilvr(torch.zeros(2, 3, 32, 32))


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from afldm_amd import ops
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ilvr_step(x, x.permute(0, 2, 3, 1).contiguous(), x, torch.zeros(1, 2, 1, 4, 4, 4), torch.eye(4), torch.eye(4),
                      torch.zeros(12), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ilvr_step_flat(x, x, x, (None, None), torch.eye(4), torch.eye(4), (1.0, 0.0, -1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0))


def test_library_refuses_planes_without_a_kernel_before_any_launch():
    """S = 65, H != W and S = 1 return AFLDM_ESHAPE with a message, and a short noise stride too: the refusal comes before
    anything touches a device, so it is checked here with made-up addresses and no GPU."""
    from afldm_amd import _lib
    lib, p = _lib.lib, 4096
    for H, W in ((65, 65), (16, 8), (8, 16), (1, 1)):
        assert lib.afldm_ilvr_step(p, p, p, p, 10 ** 6, 10 ** 5, p, p, p, p, p, 0, 1, 2, H, W, 0, None) == -1
        assert b"afldm_ilvr_step: plane %d x %d" % (H, W) in lib.afldm_last_error()
        assert lib.afldm_ilvr_step_flat(p, p, p, p, p, p, p, p, 1, 0, -1, 1, 1, 0, 0, 1, 0, 1, 2, H, W, None) == -1
        assert b"afldm_ilvr_step_flat: plane %d x %d" % (H, W) in lib.afldm_last_error()
    assert lib.afldm_ilvr_step(p, p, p, p, 100, 10 ** 5, p, p, p, p, p, 0, 1, 2, 16, 16, 0, None) == -1      # step stride < two slots
    assert lib.afldm_ilvr_step(p, p, p, p, 10 ** 6, 100, p, p, p, p, p, 0, 1, 2, 16, 16, 0, None) == -1      # slot stride < one slot
    assert lib.afldm_ilvr_step(p, p, None, p, 10 ** 6, 10 ** 5, p, p, p, p, p, 0, 1, 2, 16, 16, 0, None) == -5
    # flat: a pointer may be NULL exactly where the row does not read it
    assert lib.afldm_ilvr_step_flat(p, p, p, None, None, p, p, p, 1, 0, -1, 1, 1, 0, 0.5, 1, 0.5, 1, 2, 16, 16, None) == -5
    assert lib.afldm_ilvr_step_flat(p, p, None, None, None, p, p, p, 1, 0, -1, 1, 1, 0, 0, 1, 0, 1, 2, 16, 16, None) == -5
    assert lib.afldm_ilvr_step_flat(p, p, None, None, None, None, None, p, 1, 0, -1, 1, 1, 0, 0, 1, 0.5, 0, 0, 16, 16, None) == 0


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    for name in ("afldm_ilvr_step(", "afldm_ilvr_step_flat("):
        assert text.count("int " + name) == 1, name
    from afldm_amd import _lib
    assert _lib.lib.afldm_ilvr_step.restype is not None and len(_lib.lib.afldm_ilvr_step.argtypes) == 18
    assert len(_lib.lib.afldm_ilvr_step_flat.argtypes) == 22


def test_ilvr_script_arguments():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ilvr_ffhq", os.path.join(ROOT, "scripts", "ilvr_ffhq.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["--image", "a.png", "--random-init", "--down-factor", "8", "--range-t", "200", "--eta", "0.5", "--steps", "20",
                        "--seed", "7", "--eager", "--output", "o.png"])
    assert (a.image, a.down_factor, a.range_t, a.eta, a.steps, a.seed, a.eager, a.output) == ("a.png", 8, 200, 0.5, 20, 7, True, "o.png")
    d = mod.parse_args(["--random-init"])
    assert (d.down_factor, d.range_t, d.eta, d.steps, d.eager, d.image) == (4, 0, 1.0, 50, False, None)
    for bad in ([], ["--ckpt", "x", "--random-init"], ["--random-init", "--down-factor", "0"], ["--random-init", "--steps", "0"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    image = mod.synthetic_image(3, 64)
    assert tuple(image.shape) == (1, 3, 64, 64) and image.abs().max() <= 1
