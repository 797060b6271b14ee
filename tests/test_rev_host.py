"""The bit-reversible sampler, host side (no GPU): the numpy oracle of encode / decode / step (tests/rev_oracle.py) on the
properties the GPU tests then hold the kernels to - the inverse of a trajectory reproduces every state, image -> invert -> sample
returns the image's integers - DDIMScheduler.reversible_schedule's four row tables against the float64 formulas, the kind's
registration, the C ABI, the refusals, ReversibleCode's round trip through torch.save, and the script's options."""
import inspect
import io
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import rev_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sched(**kw):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    return DDIMScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)


def toy_eps(x, t):
    """An analytic stand-in for the UNet: deterministic fp32, depends on the state and the timestep."""
    return (np.sin(x * np.float32(1.7) + np.float32(t) / np.float32(300.0)) * np.float32(0.9)).astype(np.float32)


def tables(N, strength=None):
    s = sched()
    return {(d, c): s.reversible_schedule(N, d, c, strength) for d in ("sample", "invert") for c in (False, True)}


# ------------------------------------------------------------------------------------------------ oracle
def test_oracle_encode_decode():
    x = np.array([0.0, 2.0 ** -33, -2.0 ** -33, 3 * 2.0 ** -33, 1.5, -1.5, 2.0 ** 31 - 2.0 ** 7, -(2.0 ** 31 - 2.0 ** 7), 2.0 ** 31,
                  -2.0 ** 31, np.nan, np.inf], dtype=np.float32)
    X, bad = ro.encode(x)
    assert X.tolist() == [0, 0, 0, 2, 3 << 31, -(3 << 31), (2 ** 31 - 2 ** 7) << 32, -((2 ** 31 - 2 ** 7) << 32), 0, 0, 0, 0]
    assert bad.tolist() == [False] * 8 + [True] * 4
    # decode: ties of the int64 -> fp32 rounding go to even, and the scale is exact
    Xs = np.array([0, 1, -1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 53 + 1, 2 ** 62], dtype=np.int64)
    want = [0.0, 2.0 ** -32, -2.0 ** -32, 2.0 ** -8, (2.0 ** 24 + 4) * 2.0 ** -32, -2.0 ** -8, 2.0 ** 21, 2.0 ** 30]
    assert ro.decode(Xs).tolist() == want and ro.decode(Xs).dtype == np.float32


def test_oracle_step_is_undone_by_the_opposite_sign_and_flags_trouble():
    rng = np.random.default_rng(3)
    far = rng.integers(-2 ** 34, 2 ** 34, size=40, dtype=np.int64)
    near = rng.integers(-2 ** 34, 2 ** 34, size=40, dtype=np.int64)
    eps = rng.standard_normal(40).astype(np.float32)
    for sign in (1, -1):
        f1, n1, lat, bad = ro.step(far, near, eps, (0.7, -1.3, sign, 0))
        assert not bad.any() and np.array_equal(f1, near) and np.array_equal(lat, ro.decode(n1)) and not np.array_equal(n1, far)
        # the inverse: the same row, the other sign, the pair swapped (eps belongs to the state that is `near` again)
        f2, n2, _, bad = ro.step(n1, f1, eps, (0.7, -1.3, -sign, 0))
        assert not bad.any() and np.array_equal(n2, far) and np.array_equal(f2, near)
    # boot reads near in far's place
    _, nb, _, _ = ro.step(far, near, eps, (0.7, -1.3, 1, 1))
    _, nn, _, _ = ro.step(near, near, eps, (0.7, -1.3, 1, 0))
    assert np.array_equal(nb, nn)
    # trouble: NaN / inf eps, a product past 2^63, an add that overflows - q = 0 there, the others as without
    e = eps.copy()
    e[[1, 5, 9]] = [np.nan, np.inf, 4.0e9]          # (1.3 * 4e9 >= 2^31: finite, but past the grid)
    n2 = near.copy()
    f2 = far.copy()
    f2[20], n2[20] = 2 ** 63 - 5, 2 ** 40
    _, got, _, bad = ro.step(f2, n2, e, (0.7, 1.3, 1, 0))
    _, clean, _, _ = ro.step(far, near, eps, (0.7, 1.3, 1, 0))
    hit = [1, 5, 9, 20]
    assert np.flatnonzero(bad).tolist() == hit and np.array_equal(got[hit], f2[hit])
    keep = np.setdiff1d(np.arange(40), hit)
    assert np.array_equal(got[keep], clean[keep])


@pytest.mark.parametrize("N,strength", [(2, None), (3, None), (7, None), (50, None), (10, 0.5)])
def test_oracle_round_trips_on_all_four_tables(N, strength):
    tb = tables(N, strength)
    levels = len(tb["sample", False].rows)
    assert levels == (N if strength is None else int(N * strength))
    rows = {k: ro.f32_rows(v) for k, v in tb.items()}
    ts = {k: v.timesteps for k, v in tb.items()}
    rng = np.random.default_rng(N)
    # noise -> sample: S[k] = X_k for k = levels .. 0
    XN, bad = ro.encode(rng.standard_normal((2, 3, 5, 5)).astype(np.float32))
    assert not bad.any()
    states, far = ro.run(rows["sample", False], ts["sample", False], toy_eps, XN)
    S = {levels: XN, **{levels - 1 - i: s for i, s in enumerate(states)}}
    assert len(states) == levels and np.array_equal(far, S[1])
    # invert the code (X_1, X_0): every stored state comes back, and the noise's integers at the end
    back, far = ro.run(rows["invert", True], ts["invert", True], toy_eps, S[1], far=S[0])
    assert len(back) == levels - 1
    for i, s in enumerate(back):
        assert np.array_equal(s, S[2 + i]), (N, 2 + i)
    assert np.array_equal(back[-1], XN) and np.array_equal(far, S[levels - 1])
    # sampling from the code (X_N, X_N-1) is the from-noise run without its first row
    again, _ = ro.run(rows["sample", True], ts["sample", True], toy_eps, S[levels - 1], far=XN)
    assert len(again) == levels - 1 and all(np.array_equal(a, b) for a, b in zip(again, states[1:]))
    # image -> invert -> sample: X_0 exactly, and every state of the way up on the way down
    X0, _ = ro.encode((rng.standard_normal((2, 3, 5, 5)) * 0.8).astype(np.float32))
    up, far = ro.run(rows["invert", False], ts["invert", False], toy_eps, X0)
    assert len(up) == levels
    down, far1 = ro.run(rows["sample", True], ts["sample", True], toy_eps, far, far=up[-1])
    want = up[:-2][::-1] + [X0]
    assert len(down) == len(want) and all(np.array_equal(a, b) for a, b in zip(down, want))
    assert np.array_equal(down[-1], X0) and np.array_equal(far1, up[0])


# ------------------------------------------------------------------------------------------------ rows
def _levels(s, N, strength=None):
    """tau ascending and ab per level, restated: level 0 is final_alpha_cumprod."""
    if strength is None:
        s.set_timesteps(N)
        ts = [int(t) for t in s.timesteps]
    else:
        s.set_timesteps(N)
        ts = [int(t) for t in s.timesteps][N - min(int(N * strength), N):]
    tau = sorted(ts)
    return [None] + tau, [float(s.final_alpha_cumprod)] + [float(s.alphas_cumprod[t]) for t in tau]


def _AB(ab, k, j):
    A = math.sqrt(ab[j] / ab[k])
    return A, math.sqrt(1 - ab[j]) - A * math.sqrt(1 - ab[k])


def _one_rounding(got, want):
    return float(np.float32(want)) == got or abs(got - want) <= 2.0 ** -24 * abs(want)


@pytest.mark.parametrize("one", [True, False])
@pytest.mark.parametrize("N,strength", [(2, None), (6, None), (50, None), (6, 0.5), (50, 0.58)])
def test_rows_are_the_formulas(N, strength, one):
    s = sched(set_alpha_to_one=one)
    tau, ab = _levels(sched(set_alpha_to_one=one), N, strength)
    L = len(tau) - 1
    assert ab[0] == float(s.final_alpha_cumprod) and (ab[0] == 1.0) == one and tau[1:] == sorted(tau[1:])

    def interior(k):
        (Ad, Bd), (Au, Bu) = _AB(ab, k, k - 1), _AB(ab, k, k + 1)
        return Ad - Au, Bd - Bu

    A, B = _AB(ab, L, L - 1)
    want_sample = [(tau[L], A - 1, B, 1.0, 1.0)] + [(tau[k],) + interior(k) + (1.0, 0.0) for k in range(L - 1, 0, -1)]
    A, B = _AB(ab, 0, 1)
    want_invert = [(tau[1], A - 1, B, 1.0, 1.0)] + [(tau[k],) + interior(k) + (-1.0, 0.0) for k in range(1, L)]
    for direction, want in (("sample", want_sample), ("invert", want_invert)):
        for from_code in (False, True):
            sd = s.reversible_schedule(N, direction, from_code, strength)
            w = want[1:] if from_code else want
            assert sd.kind == "rev" and len(sd.rows) == len(w) == (L - 1 if from_code else L) and not any(sd.draws)
            assert list(sd.timesteps) == [r[0] for r in w]
            table = sd.table("cpu")
            assert table.dtype == torch.float32 and tuple(table.shape) == (len(w), 4)
            for got, row, r in zip(table.tolist(), sd.rows, w):
                assert _one_rounding(got[0], r[1]) and _one_rounding(got[1], r[2]), (direction, from_code, got, r)
                assert abs(row[0] - r[1]) <= 1e-12 and abs(row[1] - r[2]) <= 1e-12          # float64 before the one rounding
                assert got[2:] == list(r[3:]) and row[2:] == r[3:]
    # the evaluation at level 0 uses tau_1, and the boot row of sampling is the plain DDIM step from the last level
    inv = s.reversible_schedule(N, "invert", False, strength)
    assert inv.timesteps[0] == inv.timesteps[1 if L > 1 else 0] == tau[1]


def test_key_holds_every_setting():
    a = sched().reversible_schedule(6, "sample", False)
    assert sched().reversible_schedule(6, "sample", False) is a
    keys = {sched().reversible_schedule(*args).key for args in [(6, "sample", False), (6, "sample", True), (6, "invert", False),
                                                                 (6, "invert", True), (7, "sample", False), (6, "sample", False, 0.5),
                                                                 (6, "sample", False, 1.0)]}
    assert len(keys) == 7
    assert len({sched(beta_end=0.02).reversible_schedule(6, "sample", False).key, a.key}) == 2
    d = dict(a.key[1])
    assert (d["_rev_steps"], d["_rev_direction"], d["_rev_from_code"], d["_rev_strength"]) == ("6", "'sample'", "False", "None")
    assert not any(k.startswith("_rev") for k, _ in sched().schedule(6).key[1])


def test_schedule_refusals():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    with pytest.raises(NotImplementedError):
        sched(clip_sample=True).reversible_schedule(6, "sample", False)
    with pytest.raises(NotImplementedError):
        sched(prediction_type="v_prediction").reversible_schedule(6, "sample", False)
    with pytest.raises(NotImplementedError):
        sched().reversible_schedule(6, "sample", False, eta=0.5)
    with pytest.raises(ValueError):
        sched().reversible_schedule(6, "sideways", False)
    with pytest.raises(ValueError):
        sched().reversible_schedule(1, "sample", True)                    # a code needs two levels
    with pytest.raises(ValueError):
        sched().reversible_schedule(6, "invert", False, 0.1)              # int(6 * 0.1) = 0 levels
    assert not hasattr(DPMSolverMultistepScheduler, "reversible_schedule")
    dp = _pipe(DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG))
    z = torch.zeros(1, 4, 8, 8)
    for call in (lambda: dp.sample_reversible_latents(latents=z), lambda: dp.sample_reversible(latents=z),
                 lambda: dp.invert_reversible(z)):
        with pytest.raises(NotImplementedError, match="DPMSolverMultistepScheduler"):
            call()
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    for f in (I2SBLDMPipeline.sample_reversible, I2SBLDMPipeline.sample_reversible_latents, I2SBLDMPipeline.invert_reversible):
        with pytest.raises(NotImplementedError, match="I2SBLDMPipeline"):
            f(object(), z)


# ------------------------------------------------------------------------------------------------ registration and ABI
def test_kind_is_registered_with_one_engine_only():
    from afldm_amd import engine, ops
    from afldm_amd.engine import DenoiseEngine, ReversibleEngine
    from afldm_amd.schedulers.schedule import KINDS, NOISE_SLOTS, ROW_WIDTH
    assert KINDS["rev"] == (4, 1, False) and ROW_WIDTH["rev"] == 4 and "rev" not in NOISE_SLOTS
    assert issubclass(ReversibleEngine, DenoiseEngine) and ReversibleEngine.ONE_BRANCH
    assert list(ReversibleEngine.UPDATES) == ["rev"] and ReversibleEngine.UPDATES["rev"][0] is ops.rev_step
    others = [c for c in vars(engine).values() if inspect.isclass(c) and issubclass(c, DenoiseEngine) and c is not ReversibleEngine]
    assert len(others) >= 9
    for other in others:
        assert "rev" not in other.UPDATES, other
    for name in ("_carried", "reset", "_result", "check_errors"):
        assert name in vars(ReversibleEngine), name


PARAMS = {
    "afldm_rev_step": ["long long* far", "long long* near", "const void* eps", "float* lat_out", "int* bad", "const float* coef",
                       "int* step_idx", "int advance", "int B", "int C", "int H", "int W", "int dtype", "afldm_stream_t stream"],
    "afldm_rev_step_flat": ["long long* far", "long long* near", "const float* eps", "float* lat_out", "int* bad", "float cx",
                            "float ce", "int sign", "int boot", "size_t n", "size_t rows_per_sample", "afldm_stream_t stream"],
    "afldm_rev_encode": ["const float* x", "long long* X", "int* bad", "size_t n", "size_t per_sample", "afldm_stream_t stream"],
}


def test_entry_points_are_declared_bound_exported_and_documented():
    from ctypes import c_float, c_int, c_size_t, c_void_p
    from afldm_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(ROOT, "afldm_amd", "csrc", "rev.hip")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    kinds = {"float": c_float, "int": c_int, "size_t": c_size_t}
    for name, params in PARAMS.items():
        decl = re.search(r"int " + name + r"\(([^;]*)\);", hdr)
        assert decl, name
        assert [" ".join(p.split()) for p in decl.group(1).split(",")] == params
        fn = getattr(_lib.lib, name)
        want = [c_void_p if "*" in p or p.startswith("afldm_stream_t") else kinds[p.rsplit(" ", 1)[0]] for p in params]
        assert fn.argtypes == want and fn.restype is c_int, name
        assert name in _lib.EXPORTS and re.search(r" T " + name + "$", nm, re.M) and name in doc
        assert 'extern "C" int ' + name + "(" in src
    assert "rev.hip" in build.SOURCES
    assert re.fullmatch(r"[0-9a-f]{64}", _lib.library_hash()) and _lib.library_hash() is _lib.library_hash()


def test_cpu_tensors_are_refused():
    from afldm_amd import ops
    X = torch.zeros(1, 4, 4, 4, dtype=torch.int64)
    x = torch.zeros(1, 4, 4, 4)
    bad = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rev_step(X, X.clone(), x.permute(0, 2, 3, 1).contiguous(), bad, torch.zeros(4), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rev_step_flat(X, X.clone(), x, bad, (1.0, 0.0, 1, 0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rev_encode(x, bad)
    pipe = _pipe()
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.sample_reversible_latents(latents=torch.zeros(1, 4, 8, 8), num_inference_steps=4, use_graph=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.invert_reversible(torch.zeros(1, 4, 8, 8), num_inference_steps=4)


# ------------------------------------------------------------------------------------------------ pipeline surface
class _FakeUnet(torch.nn.Module):
    dtype, device = torch.float32, torch.device("cpu")

    class config:
        in_channels, sample_size = 4, 8

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def _pipe(scheduler=None):
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    pipe = MyLDMPipeline(None, _FakeUnet(), scheduler or sched())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def test_pipeline_surface():
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    import afldm.pipelines.ldm_pipeline as alias
    import afldm.reversible as alias_code
    from afldm_amd.reversible import ReversibleCode
    assert alias.MyLDMPipeline.sample_reversible is MyLDMPipeline.sample_reversible and alias_code.ReversibleCode is ReversibleCode
    p = inspect.signature(MyLDMPipeline.sample_reversible).parameters
    assert list(p)[1:10] == ["batch_size", "num_inference_steps", "generator", "latents", "code", "output_type", "return_dict",
                             "use_graph", "return_code"]
    assert [p[k].default for k in list(p)[1:10]] == [1, 50, None, None, None, "pil", True, True, False] and p["exact"].default is True
    p = inspect.signature(MyLDMPipeline.invert_reversible).parameters
    assert list(p)[1:6] == ["image_or_latents", "code", "num_inference_steps", "strength", "use_graph"]
    assert [p[k].default for k in list(p)[1:6]] == [None, None, 50, None, True]
    assert "eta" not in inspect.signature(MyLDMPipeline.sample_reversible_latents).parameters
    pipe = _pipe()
    with pytest.raises(ValueError):
        pipe.invert_reversible()                                           # neither an image nor a code
    with pytest.raises(ValueError):
        pipe.sample_reversible_latents(latents=torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="without a VAE"):
        pipe.invert_reversible(torch.zeros(1, 3, 32, 32))
    with pytest.raises(TypeError):
        pipe.sample_reversible_latents(num_inference_steps=4, eta=0.5)     # there is no eta to pass


def _code(pipe, k, steps=4, rows=2, **kw):
    from afldm_amd import _lib
    from afldm_amd.engine import model_state_key
    from afldm_amd.reversible import ReversibleCode
    X = torch.arange(rows * 4 * 8 * 8, dtype=torch.int64).reshape(rows, 4, 8, 8)
    f = dict(hi=X, lo=X + 1, k=k, num_inference_steps=steps, strength=None, batch=rows, dtype=pipe.unet.dtype,
             model_key=model_state_key(pipe.unet), library=_lib.library_hash())
    f.update(kw)
    return ReversibleCode(**f)


def test_mismatched_codes_are_refused_field_by_field():
    pipe = _pipe()
    # a matching code passes the checks and only then meets the missing GPU
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.sample_reversible_latents(code=_code(pipe, 4), num_inference_steps=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.invert_reversible(code=_code(pipe, 1), num_inference_steps=4)
    for field, value in (("batch", 3), ("dtype", torch.bfloat16), ("model_key", 12345), ("library", "0" * 64),
                         ("num_inference_steps", 5)):
        steps, k = 4, 4
        with pytest.raises(ValueError, match=field):
            pipe.sample_reversible_latents(code=_code(pipe, k, **{field: value}), num_inference_steps=steps)
        with pytest.raises(ValueError, match=field):
            pipe.invert_reversible(code=_code(pipe, 1, **{field: value}), num_inference_steps=steps)
        with pytest.raises(RuntimeError, match="no CPU path"):            # exact=False lets it through
            pipe.sample_reversible_latents(code=_code(pipe, k, **{field: value}), num_inference_steps=steps, exact=False)
    # the level is checked whatever `exact` says: a code at the image end cannot be sampled from, and the other way round
    for exact in (True, False):
        with pytest.raises(ValueError, match="level"):
            pipe.sample_reversible_latents(code=_code(pipe, 1), num_inference_steps=4, exact=exact)
        with pytest.raises(ValueError, match="level"):
            pipe.invert_reversible(code=_code(pipe, 4), num_inference_steps=4, exact=exact)
    with pytest.raises(TypeError):
        pipe.sample_reversible_latents(code=torch.zeros(2, 4, 8, 8), num_inference_steps=4)
    with pytest.raises(ValueError):
        pipe.sample_reversible_latents(code=_code(pipe, 4), latents=torch.zeros(2, 4, 8, 8), num_inference_steps=4)
    # a slice keeps the batch size that made the bits, so it is refused unless exact=False
    with pytest.raises(ValueError, match="batch"):
        pipe.sample_reversible_latents(code=_code(pipe, 4)[:1], num_inference_steps=4)


def test_code_round_trips_through_torch_save():
    pipe = _pipe()
    code = _code(pipe, 4, strength=0.5, dtype=torch.bfloat16)
    buf = io.BytesIO()
    torch.save(code, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert type(back) is type(code) and torch.equal(back.hi, code.hi) and torch.equal(back.lo, code.lo)
    assert (back.k, back.num_inference_steps, back.strength, back.batch, back.dtype, back.model_key, back.library) == (
        code.k, code.num_inference_steps, code.strength, code.batch, code.dtype, code.model_key, code.library)
    assert back.cpu().hi.device.type == "cpu" and back.to("cpu").k == 4
    lat = code.latents()
    assert lat.dtype == torch.float32 and np.array_equal(lat.numpy(), ro.decode(code.lo.numpy()))
    one = code[1]
    assert tuple(one.hi.shape) == (1, 4, 8, 8) and one.batch == 2 and torch.equal(one.lo, code.lo[1:2])


def test_script_parses_its_options():
    import importlib.util
    script = os.path.join(ROOT, "scripts", "invert_ffhq.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--ckpt", "--random-init", "--image", "--from-noise", "--steps", "--strength"):
        assert flag in r.stdout, flag
    spec = importlib.util.spec_from_file_location("invert_ffhq", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["--random-init", "--steps", "8", "--strength", "0.5"])
    assert (a.steps, a.strength, a.from_noise, a.image, a.random_init) == (8, 0.5, False, None, True)
    assert mod.parse_args(["--ckpt", "dir", "--from-noise"]).from_noise
    for bad in ([], ["--from-noise"], ["--ckpt", "dir"], ["--random-init", "--steps", "1"], ["--random-init", "--strength", "1.5"],
                ["--random-init", "--from-noise", "--strength", "0.5"], ["--random-init", "--from-noise", "--image", "a.png"],
                ["--random-init", "--steps", "8", "--strength", "0.2"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    assert mod.psnr(torch.zeros(3), torch.zeros(3)) == math.inf and abs(mod.psnr(torch.zeros(4), torch.ones(4)) - 10 * math.log10(4)) < 1e-12
