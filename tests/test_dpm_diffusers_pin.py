"""Opportunistic pin of DPMSolverMultistepScheduler's coefficient rows against the REAL
`diffusers.DPMSolverMultistepScheduler` step outputs (on CPU tensors, in diffusers' own float32 arithmetic).  diffusers is
not installed in the build image, so this skips there, like tests/test_diffusers_pin.py.  Nothing here touches a GPU."""
import pytest
import torch

from test_dpm_host import apply_rows

pytestmark = pytest.mark.gpu          # as tests/test_diffusers_pin.py: also runs wherever `-m gpu` is the suite

diffusers = pytest.importorskip("diffusers", reason="diffusers is not installed here: the DPM-Solver rows stay unpinned")
if getattr(diffusers, "__afldm_shim__", False):
    pytest.skip("only afldm_amd's own diffusers shim is importable", allow_module_level=True)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("algo,final", [("dpmsolver++", "zero"), ("dpmsolver++", "sigma_min"), ("dpmsolver", "sigma_min")])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_rows_match_diffusers_steps(order, algo, final, pred):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    kw = dict(solver_order=order, algorithm_type=algo, final_sigmas_type=final, prediction_type=pred)
    real = diffusers.DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)
    ours = DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)
    for n in (10, 20):
        real.set_timesteps(n)
        ours.set_timesteps(n)
        assert real.timesteps.tolist() == ours.timesteps.tolist()
        g = torch.Generator().manual_seed(n + order)
        x = torch.randn(1, 4, 8, 8, generator=g)
        outs = [torch.randn(1, 4, 8, 8, generator=g) for _ in range(n)]
        got = apply_rows(ours.coefficient_table("cpu").double(), x.double(), [o.double() for o in outs])
        z = x
        for i, t in enumerate(real.timesteps):
            z = real.step(outs[i], t, z).prev_sample
            err = float((got[i] - z.double()).abs().max() / z.double().abs().max())
            assert err <= 1e-4, (n, i, err)
