"""The alias-free activation's and resampler's planners on the host (afldm_af_act_route / afldm_af_resample_route with
cus = 256: no GPU).  Guards the claim "this route is tested": every activation site of the FFHQ AF-UNet, at every benchmark
batch size and in both dtypes, must plan into a route that tests/test_gpu_af_routes.py compares with the float64 oracle
(its COVERED set), and the facts about the planner that the choice of cases there rests on are asserted one by one."""
import pytest
import torch

from test_gpu_af_routes import COVERED, FFHQ_AF_ACT_SITES, PLANE_INST, route_key
from test_gpu_groupnorm_stats import AF_SHAPES

CUS = 256
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
BATCHES = [1, 8, 16, 32, 64]


def _ops():
    from afldm_amd import ops
    return ops


def _route(dtype, N, C1, C2, B):
    return _ops().af_act_route(dtype, N, C1, C2, B, cus=CUS)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_ffhq_site_plans_into_a_tested_route(dtype, B):
    for N, C1, C2 in FFHQ_AF_ACT_SITES:
        r = _route(dtype, N, C1, C2, B)
        assert route_key(dtype, N, r) in COVERED, f"site N={N} {C1}|{C2} at batch {B}: {r} is compared with no reference"


def test_covered_holds_every_plane_instantiation_both_ways():
    for dtype, N, CH in PLANE_INST:
        for several in (False, True):
            assert (str(dtype).replace("torch.", ""), N, "plane", CH, several) in COVERED


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_planner_facts_the_gpu_cases_rest_on(dtype):
    # 4 x 4 planes run the VALU kernel by default, whatever the channel count
    for B in BATCHES:
        assert _route(dtype, 4, 768, 0, B).kernel == "small"
        assert _route(dtype, 4, 96, 48, B).kernel == "small"
    # 8 x 8: bf16 on the separable kernel, fp32 on the Kronecker kernel, both only with whole 16-channel items
    for C1, C2 in ((96, 48), (64, 0), (384, 384)):
        assert _route(dtype, 8, C1, C2, 3).kernel == ("p8" if dtype == BF16 else "kron")
    assert _route(dtype, 8, 24, 12, 3).kernel == "small"
    assert _route(dtype, 2, 64, 0, 3).kernel == "small"
    # the B = 3 rows of AF_SHAPES never reach the 16-channel items of the plane kernel, nor a second item per workgroup
    for N, C1, C2, _ in AF_SHAPES:
        if N >= 16:
            r = _route(dtype, N, C1, C2, 3)
            assert (r.kernel, r.ch, r.items_per_wg) == ("plane", 8, 1), (N, C1, C2, r)
    # ... which the benchmark's batch-64 sites above 40 MB do
    r = _route(dtype, 32, 192, 192, 64)
    assert r.kernel == "plane" and r.ch == 16 and r.items_per_wg > 1, r
    r = _route(F32, 32, 192, 0, 64)
    assert r.kernel == "plane" and r.ch == 16 and r.items_per_wg > 1, r


def test_planner_grid_and_items_per_workgroup():
    ops = _ops()
    assert _route(BF16, 32, 192, 192, 64) == ("plane", 16, 512, 3)          # 2 workgroups per CU, 1536 items
    assert _route(BF16, 16, 384, 0, 64) == ("plane", 8, 1024, 3)            # 4 per CU, 3072 items
    assert _route(F32, 8, 16, 0, 5) == ("kron", 0, 2, 4)                    # 5 items in groups of four
    assert _route(BF16, 8, 16, 0, 5) == ("p8", 0, 2, 4)
    assert _route(F32, 2, 100, 0, 3) == ("small", 0, 2, 256)
    with pytest.raises(RuntimeError, match="afldm_af_act_route: plane size N=3"):
        _route(F32, 3, 16, 0, 1)
    with pytest.raises(RuntimeError, match="multiples of 16"):
        _route(F32, 16, 24, 0, 1)
    assert ops.af_act_route(F32, 4, 96, 48, 3, cus=CUS, has_packed=False).kernel == "small"


def test_af_tune_sets_one_field_and_always_resets():
    ops = _ops()
    base = [_route(d, N, 64, 0, 2) for d in DTYPES for N in (4, 8, 16, 32)]
    with ops.af_tune(small_n=0):
        assert _route(F32, 4, 64, 0, 2).kernel == "kron" and _route(F32, 4, 36, 0, 2).kernel == "small"
    with ops.af_tune(small_n=12):
        assert _route(BF16, 8, 64, 0, 2).kernel == "small" and _route(F32, 8, 64, 0, 2).kernel == "small"
    with ops.af_tune(p8=0):
        assert _route(BF16, 8, 64, 0, 2).kernel == "kron"
    for CH in (8, 16):
        with ops.af_tune(ch=CH, max_grid=2):
            for d in DTYPES:
                for N in (16, 32):
                    assert _route(d, N, 64, 0, 2) == ("plane", CH, 2, 64 // CH)
    with pytest.raises(ZeroDivisionError):
        with ops.af_tune(ch=16, max_grid=1):
            assert _route(BF16, 32, 64, 0, 2) == ("plane", 16, 1, 8)
            1 // 0
    assert [_route(d, N, 64, 0, 2) for d in DTYPES for N in (4, 8, 16, 32)] == base
    for bad in (dict(ch=4), dict(small_n=3), dict(resample_split=3), dict(max_grid=-1), dict(stagger=-1)):
        with pytest.raises(RuntimeError, match="afldm_af_tune"):
            with ops.af_tune(**bad):
                pass
    with pytest.raises(TypeError):
        with ops.af_tune(chh=8):
            pass


def test_environment_variables_are_the_defaults_af_tune_resets_to():
    """The tuning struct is filled from the environment once per process: a fresh interpreter with the variables set plans as
    they say, before and after an af_tune block."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, torch\n"
            "from afldm_amd import ops\n"
            "def routes():\n"
            "    return [list(ops.af_act_route(torch.bfloat16, N, 64, 0, 2, cus=256)) for N in (4, 8, 32)] + "
            "[list(ops.af_resample_route(4, 64, 8)), list(ops.af_resample_route(16, 64, 8))]\n"
            "a = routes()\n"
            "with ops.af_tune(ch=8, small_n=12, p8=1, no_resample_small=0, resample_split=2, max_grid=1):\n"
            "    b = routes()\n"
            "print(json.dumps([a, b, routes()]))\n")
    env = dict(os.environ, AFLDM_AF_CH="16", AFLDM_AF_SMALL_N="0", AFLDM_AF_P8="0", AFLDM_NO_RESAMPLE_SMALL="1",
               AFLDM_RESAMPLE_SPLIT="2", AFLDM_AF_STAGGER="0")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True).stdout
    a, b, c = json.loads(out.strip().splitlines()[-1])
    assert a == c == [["kron", 0, 2, 4], ["kron", 0, 2, 4], ["plane", 16, 8, 1], ["reg", 0], ["reg", 0]]
    assert b == [["small", 0, 1, 128], ["small", 0, 1, 128], ["plane", 8, 1, 16], ["small", 1], ["reg", 0]]


def test_resample_routes():
    ops = _ops()
    small = {(2, 4): 1, (4, 8): 1, (8, 16): 4, (4, 2): 1, (8, 4): 1}
    for (N, R), split in small.items():
        for C in (4, 64, 100, 6):
            assert ops.af_resample_route(N, C, R) == ("small", split)
        with ops.af_tune(no_resample_small=1):
            assert ops.af_resample_route(N, 100, R) == ("reg", 0)
            assert ops.af_resample_route(N, 6, R) == ("generic", 0)           # the register-blocked passes own 4 channels
    for split in (1, 2, 4):
        with ops.af_tune(resample_split=split):
            assert ops.af_resample_route(8, 64, 16) == ("small", split)
            assert ops.af_resample_route(4, 64, 8) == ("small", 1)
    assert ops.af_resample_route(16, 64, 8) == ("reg", 0) and ops.af_resample_route(16, 64, 32) == ("reg", 0)
    assert ops.af_resample_route(32, 64, 16) == ("reg", 0)
    for N, R in ((32, 64), (2, 1), (16, 16), (16, 128), (12, 24)):
        assert ops.af_resample_route(N, 64, R) == ("generic", 0)
