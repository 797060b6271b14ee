"""DPM-Solver(++) multistep sampling on MI355X: the update kernels (afldm_dpm_step, afldm_dpm_step_flat) against a torch
restatement, DenoiseEngine over DPMSolverMultistepScheduler's rows against the CPU oracle UNet driven by the float64
restated solver of tests/test_dpm_host.py, and the pipeline opt-in.  Bounds: the DDIM trajectory tests' (fp32 1e-3,
bf16 5e-2 rel-RMS)."""
import numpy as np
import pytest
import torch

from test_dpm_host import RefSolver, ref_sigmas, ref_timesteps

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def rel_rms(got, ref):
    got, ref = got.double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def build(cfg_name, dtype):
    from afldm_amd.af_modules.af_api import make_af_unet
    from afldm_amd.models.unet_2d import UNet2DModel
    from oracle import configs as oc, unet as ou
    if cfg_name == "tiny":
        cfg = oc.tiny_unet()
        sd = ou.randomize_norm_affine(ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1))
    else:
        cfg = oc.FFHQ_UNET
        sd = ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1)
    unet = UNet2DModel.from_config(cfg)
    unet.load_state_dict(sd)
    make_af_unet(unet)
    return unet.to("cuda").to(dtype), cfg, sd


def _run_across_a_dtype_change(make, x):
    """run on the fp32 UNet, unet.to(bfloat16), run again on the same engine: (engine, whether refresh_if_stale said the model moved,
    the second result, the result of an engine newly made on the bf16 UNet)."""
    eng = make()
    eng.run(x)
    eng.unet.to(torch.bfloat16)
    said, plain = [], eng.refresh_if_stale
    eng.refresh_if_stale = lambda: said.append(plain()) or said[-1]
    got = eng.run(x)
    return eng, said, got, make().run(x)


def dpm(**kw):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)


def oracle_trajectory(sd, cfg, x, steps, order):
    """The oracle UNet (fp32, CPU) driven by the test module's float64 DPM-Solver++ restatement (FFHQ schedule)."""
    from oracle import unet as ou
    betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float32) ** 2
    ts = ref_timesteps(1000, steps, "leading", 1)
    ref = RefSolver(ref_sigmas(betas, ts, "zero"), order, "dpmsolver++", "midpoint", "epsilon", final="zero")
    z = x.double()
    for t in ts:
        eps = ou.unet_forward(sd, cfg, z.float(), int(t)).double()
        z = ref.step(eps, z)
    return z


# ------------------------------------------------------------------------------------------------ kernels
def torch_update(x, eps, h1, h2, row):
    p, q, a, b0, b1, b2 = [float(v) for v in row[:6]]
    m = p * x + q * eps
    return a * x + b0 * m + b1 * h1 + b2 * h2, m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 4, 8, 8), (2, 3, 5, 5)])      # 16-byte groups / the scalar form (H*W odd)
def test_dpm_step_kernel(dtype, shape):
    from afldm_amd import ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(*shape, generator=g)
    eps = torch.randn(*shape, generator=g).to(dtype).float()           # what the kernel reads
    hist = torch.randn(2, *shape, generator=g)
    coef = torch.randn(3, 8, generator=g)
    coef[:, 6:] = 0
    idx = torch.ones(1, dtype=torch.int32, device="cuda")
    xg, hg = x.cuda(), hist.cuda().contiguous()
    out = ops.dpm_step(xg, eps.permute(0, 2, 3, 1).contiguous().to("cuda", dtype), hg, coef.cuda().reshape(-1), idx,
                       advance=True, out=xg)                            # x_out aliases x
    want, m = torch_update(x.double(), eps.double(), hist[0].double(), hist[1].double(), coef[1])
    assert out.data_ptr() == xg.data_ptr() and int(idx.item()) == 2
    tol = 1e-5 * float(want.abs().max())
    assert (out.cpu().double() - want).abs().max() <= tol
    assert (hg[0].cpu().double() - m).abs().max() <= tol                # h1 <- m0
    assert torch.equal(hg[1].cpu(), hist[0])                            # h2 <- old h1


@pytest.mark.parametrize("n", [4096, 1001])
def test_dpm_step_flat_kernel(n):
    from afldm_amd import ops
    g = torch.Generator().manual_seed(12)
    x, eps, hist = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(2, n, generator=g)
    row = torch.randn(6, generator=g).tolist()
    xg, hg = x.cuda(), hist.cuda()
    out = ops.dpm_step_flat(xg, eps.cuda(), hg, row, out=xg)
    want, m = torch_update(x.double(), eps.double(), hist[0].double(), hist[1].double(), row)
    tol = 1e-5 * float(want.abs().max())
    assert (out.cpu().double() - want).abs().max() <= tol
    assert (hg[0].cpu().double() - m).abs().max() <= tol and torch.equal(hg[1].cpu(), hist[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_dpm_step_run_with_history_and_scheduler_step(dtype):
    """A 3M schedule's real rows over 8 steps: the device-indexed form, the flat form behind scheduler.step and a torch
    float64 restatement of the linear form agree while the history fills and is used."""
    from afldm_amd import ops
    s = dpm(solver_order=3)
    s.set_timesteps(8)
    table = s.coefficient_table("cuda")
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 4, 16, 16, generator=g)
    outs = [torch.randn(2, 4, 16, 16, generator=g).to(dtype).float() * 0.5 for _ in range(8)]
    xg, hist = x.cuda(), torch.zeros(2, 2, 4, 16, 16, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    xr, h1, h2 = x.double(), torch.zeros_like(x).double(), torch.zeros_like(x).double()
    xs = x.cuda()
    for i, t in enumerate(s.timesteps):
        ops.dpm_step(xg, outs[i].permute(0, 2, 3, 1).contiguous().to("cuda", dtype), hist, table.reshape(-1), idx,
                     advance=True, out=xg)
        xs = s.step(outs[i].cuda(), t, xs).prev_sample
        xr, m = torch_update(xr, outs[i].double(), h1, h2, table[i].cpu().double())
        h2, h1 = h1, m
        assert rel_rms(xg, xr) <= 1e-5 and rel_rms(xs, xr) <= 1e-5, i
    assert rel_rms(xs, xg) <= 1e-6                                      # same update; the two kernels may contract differently
    assert s.lower_order_nums == 3 and s.step_index == 8


# ------------------------------------------------------------------------------------------------ tiny UNet
@pytest.mark.parametrize("order", [2, 3])
def test_tiny_unet_dpm_20_steps_graph_eager_oracle(golden, order, monkeypatch):
    from afldm_amd.engine import DenoiseEngine
    g = golden("g6_tiny_unet.npz")
    unet, cfg, sd = build("tiny", torch.float32)
    x = torch.from_numpy(g["x"])
    eng = DenoiseEngine(unet, dpm(solver_order=order), 2, 20, use_graph=True)
    assert eng.hist is not None and eng.coef.numel() == 20 * 8
    out_graph = eng.run(x)
    eager = DenoiseEngine(unet, dpm(solver_order=order), 2, 20, use_graph=False).run(x)
    assert torch.equal(eager, out_graph), "graph replay must be bit-identical to eager launches"
    assert torch.equal(eng.run(x), out_graph), "re-running (history re-zeroed by reset) must be deterministic"
    ref = oracle_trajectory(sd, cfg, x, 20, order)
    err = rel_rms(out_graph, ref)
    print(f"[tiny DPM++ {order}M 20 steps] fp32 rel-RMS vs oracle {err:.3e}")
    assert err <= 1e-3, err
    from afldm_amd import trunk
    monkeypatch.setattr(trunk, "_BLOCKED", set(trunk._BLOCKED))       # a branched engine blocks the cooperative trunk for the
    monkeypatch.setenv("AFLDM_BRANCHES", "2")                          # process: keep that to this test
    eng2 = DenoiseEngine(unet, dpm(solver_order=order), 2, 20, use_graph=True)
    assert eng2.branches == 2 and eng2.hist.shape[:3] == (2, 2, 1)
    two = eng2.run(x)
    d = rel_rms(two, out_graph)
    print(f"[tiny DPM++ {order}M] AFLDM_BRANCHES=2 vs 1: bit-equal {torch.equal(two, out_graph)}, rel-RMS {d:.2e}")
    assert d <= 1e-5, d


# ------------------------------------------------------------------------------------------------ FFHQ-size UNet
@pytest.fixture(scope="module")
def ffhq_oracle():
    from oracle import configs as oc, unet as ou
    cfg = oc.FFHQ_UNET
    sd = ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(21))
    return x, oracle_trajectory(sd, cfg, x, 20, 2)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 5e-2)])
def test_ffhq_dpmpp_2m_20_steps_vs_oracle(ffhq_oracle, dtype, tol):
    from afldm_amd.engine import DenoiseEngine
    x, ref = ffhq_oracle
    unet, _, _ = build("ffhq", dtype)
    out = DenoiseEngine(unet, dpm(), 2, 20, use_graph=True).run(x)
    err = rel_rms(out, ref)
    print(f"[FFHQ DPM++ 2M 20 steps, batch 2] {dtype}: rel-RMS vs oracle {err:.3e}")
    assert err <= tol, err


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_dpm_opt_in_and_ddim_default(golden):
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    g = golden("g6_tiny_unet.npz")
    unet, _, _ = build("tiny", torch.float32)
    x = torch.from_numpy(g["x"])
    fresh = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    fresh.set_progress_bar_config(disable=True)
    ddim20 = fresh(latents=x, num_inference_steps=20, output_type="latent")

    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    got = pipe(latents=x, num_inference_steps=20, output_type="latent")
    assert isinstance(pipe.scheduler, DPMSolverMultistepScheduler)
    want = DenoiseEngine(unet, dpm(), 2, 20, use_graph=True).run(x)
    assert torch.equal(got, want)
    assert torch.equal(pipe(latents=x, num_inference_steps=20, output_type="latent", use_graph=False, eta=0.3), want)
    assert rel_rms(got, ddim20) > 1e-3                                  # a different sampler did run

    again = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    again.set_progress_bar_config(disable=True)
    assert torch.equal(again(latents=x, num_inference_steps=20, output_type="latent"), ddim20)
    pipe.scheduler = ffhq_ddim_scheduler()                              # back to DDIM on the same pipeline: no stale engine
    assert torch.equal(pipe(latents=x, num_inference_steps=20, output_type="latent"), ddim20)
