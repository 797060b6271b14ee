"""CPU checks of tests/fusednorm_oracle.py, the integer-plane oracle of the fused convolution -> GroupNorm -> activation launches.

  * The filter matrices the kernels are handed equal oracle.ideal_filters to fp32 rounding, and the tap sums of the plane-constant
    dense layer equal a float64 3x3 convolution of a constant 2x2 plane.
  * The conditions (caps, variance >= 1, sigma <= 12) hold for every case tests/test_gpu_fused_norm_exact.py lists, and its tables
    hold every value at least twice.
  * The float32 restatements of the three kernels (model_slabs, model_dense2, model_ynorm) stay within the tolerance after the store
    and within A / 8 = 2^-19 max|hn| of float64 before it (measured: <= 0.07 x 2^-21 max|hn| before the store, <= 0.986 of the
    tolerance after the bf16 one, 0.05 after the fp32 one).
  * Planted faults, each confined to ONE workgroup, each put elements outside the tolerance.  What the whole-tensor rel-RMS the
    older tests assert (bf16: 6e-3 against the separate launches, 1.5e-2 against fp64 for dense2; 4e-3 / 6e-3 for af_act_slabs; 2e-3
    of the whole UNet for y_norm) shows for the same fault is printed beside it and recorded in PLANTED below.
  * Coverage guard (in the style of test_af_routes_host.py): every FFHQ site that takes one of the three launches at batch 64 falls
    in a class - (dtype, channels per group, K steps per wave), (N, channels per group, nslab), the y_norm channels per group - that
    the GPU file runs.

PLANTED (bf16; elements outside the tolerance, worst error / tolerance, rel-RMS of the faulted output against the clean one):
  dense2 768 -> 768, B = 33, workgroup (group 5, row tile 1: 16 samples x 24 channels) of 96:
    kstep 317, x856, 8.3e-3      kelem 63, x48, 8.0e-4        temb_row 378, x3.7e3, 6.0e-2
    tiles 353, x597, 1.0e-2      group_stats 377, x2.1e3, 3.9e-2    gamma_beta 378, x8.7e3, 8.1e-2
  af_act_slabs 768 / 32, N = 4, act 1, five slabs, B = 3, workgroup (sample 0, groups 0 - 7) of 12:
    slab_skipped 3067, x1.4e4, 0.35    pixswap 2476, x1.1e4, 0.11    temb_row 3056, x1.9e4, 0.27
    group_stats 3062, x6.2e4, 0.82     gamma_beta 3053, x6.6e3, 0.19    residual_late 3044, x2.3e3, 0.12
  y_norm 384 -> 384, B = 41, workgroup (sample 0, couts 0 - 95) of 164:
    pixswap 180, x6.6e3, 1.2e-2    group_stats 6142, x5.0e3, 2.8e-2    gamma_beta 6122, x5.1e3, 4.1e-2
  In one batch-64 step the same workgroup is one of 128 (dense2), 2048 (af_act_slabs on 4x4 planes) and 256 (y_norm), so the
  figures scale by sqrt(96 / 128), sqrt(12 / 2048) and sqrt(164 / 256): a lost K element (7e-4) and a lost K step (7e-3) sit under
  the 1.5e-2 the fp64 comparison of dense2 allows, the slab faults at 9e-3 ... 6e-2 around the 2e-2 of the PyTorch comparison, and
  none of the y_norm faults would move the whole UNet's output by the 2e-3 its only other check allows for.
"""
import ctypes

import numpy as np
import pytest
import torch

import fusednorm_oracle as fo
from test_conv_plan_host import unet_sites
from test_gpu_fused_norm_exact import DENSE2_CLASSES, SLAB_CLASSES, YNORM_CLASSES

BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = [FP32, BF16]
CASES = fo.all_cases()


def test_filter_matrices_are_the_ideal_ones():
    from oracle import ideal_filters as idf
    for N in (2, 4):
        U, D = fo.filters(N)
        for got, want in ((U, idf.up_matrix(N, 2)), (D, idf.down_matrix(2 * N))):
            want = torch.from_numpy(np.asarray(want)).double()
            assert got.shape == want.shape
            assert float((got.double() - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max()) + 1e-12
    # D of a 2x2 plane is 1/4 everywhere: the activation's output is plane-constant
    assert torch.equal(fo.filters(2)[1], torch.full((2, 4), 0.25))


def test_tap_sums_are_the_convolution_of_a_constant_plane():
    g = torch.Generator().manual_seed(1)
    W = torch.randint(-1, 2, (12, 16, 3, 3), generator=g).double()
    a = torch.randint(-1, 2, (5, 16), generator=g).double()
    y = torch.nn.functional.conv2d(a[:, :, None, None].expand(5, 16, 2, 2), W, padding=1)      # [B, Cout, 2, 2]
    assert torch.equal((a @ fo.tap_sum_cm(W).t()).reshape(5, 12, 2, 2), y)


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_conditions_hold_for_every_listed_case(name):
    dict(CASES)[name]()           # (the builders assert check_caps, variance >= 1 and sigma <= 12 on the float64 reference)


def test_tables_hold_every_value_at_least_twice():
    def twice(rows, col, values):
        for v in values:
            assert sum(1 for r in rows if r[col] == v) >= 2, (col, v)
    d = fo.DENSE2_CASES
    twice(d, 0, (1, 16, 17, 33))
    twice(d, 1, (1, 2, 3, 4, 6, 7, 13, -768))
    twice([(r[2], r[3]) + r for r in d], 0, (64, 96, 192, 768))
    twice(d, 4, fo.TEMB_MODES)
    twice(d, 5, (True, False))
    twice(d, 6, ("conv", "ints"))
    s = fo.SLAB_CASES
    twice(s, 0, fo.SLAB_NSLAB)
    twice(s, 1, (2, 4))
    twice(s, 2, (0, 1, 2))
    twice([((r[3], r[4]),) for r in s], 0, fo.SLAB_CG)
    twice(s, 5, fo.TEMB_MODES)
    for col in (6, 7, 8):
        twice(s, col, (True, False))
    assert all(r[1] == 2 for r in s if r[2] == 2)
    # every (nslab, N) and every (act, N) pair that exists is there
    assert {(r[0], r[1]) for r in s} >= {(z, N) for z in fo.SLAB_NSLAB for N in (2, 4)}


def _a8(pre, ref, hn):
    """|pre - ref| / (A / 8) of the restatement before its store."""
    return float((pre.double().reshape(ref.shape) - ref).abs().max()) / (2.0 ** -19 * float(hn.abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_restatements_stay_within_the_tolerance(dtype):
    worst = {"slabs": [0, 0], "dense2": [0, 0], "ynorm": [0, 0]}

    def note(kind, pre, stored, ref, hn, what):
        r8 = _a8(pre, ref, hn)
        assert r8 <= 1.0, f"{what}: the restatement is {r8:.3g} x A / 8 from float64 before the store"
        w = fo.check_elements(stored, ref, hn, dtype, what)
        worst[kind] = [max(worst[kind][0], r8 / 4), max(worst[kind][1], w)]        # (r8 / 4: in units of 2^-21 max|hn|)

    for row in fo.SLAB_CASES:
        c = fo.slab_case(*row)
        pre, stored, raw = fo.model_slabs(c, dtype)
        assert torch.equal(raw.double(), c.y), c.what
        note("slabs", pre, stored, c.ref, c.hn, c.what)
    for row in fo.DENSE2_CASES:
        c = fo.dense2_case(*row, dtype)
        pre, stored = fo.model_dense2(c)
        note("dense2", pre, stored, c.ref, c.hn, c.what)
    if dtype == BF16:
        for row in fo.YNORM_CASES:
            c = fo.ynorm_case(*row)
            pre, stored = fo.model_ynorm(c)
            note("ynorm", pre, stored, c.hn, c.hn, c.what)
    print(f"[fusednorm host] {dtype}: worst (error before the store / 2^-21 max|hn|, error / tolerance after it): {worst}")


def _planted(clean, faulty, region, ref, hn, what):
    """The fault confined to `region` (index into [B, ..., C]); -> (elements outside the tolerance, worst ratio, rel-RMS)."""
    out = clean.clone()
    out[region] = faulty[region]
    ratio = (out.double().reshape(ref.shape) - ref).abs() / fo.tolerance(ref, hn, BF16)
    n, w, r = int((ratio > 1).sum()), float(ratio.max()), fo.rel_rms(out, clean)
    print(f"[fusednorm host] planted {what}: {n} elements outside, worst error / tolerance {w:.3g}, rel-RMS against the clean output {r:.2e}")
    assert n >= 1, f"{what}: the planted fault stays inside the tolerance"
    return n, w, r


def test_planted_faults_in_dense2_leave_the_tolerance():
    c = fo.dense2_case(33, -768, 768, 32, "cout", True, "conv", BF16)
    where = (5, 2, 1)                                   # group 5, its tile 2, row tile 1 (samples 16 - 31)
    _, clean = fo.model_dense2(c)
    assert fo.check_elements(clean, c.ref, c.hn, BF16) <= 1.0
    everywhere = (slice(None),)
    seen = {}
    for fault in ("kstep", "kelem", "temb_row", "tiles", "group_stats", "gamma_beta"):
        _, bad = fo.model_dense2(c, fault, where)       # (already confined to the workgroup by the model)
        seen[fault] = _planted(clean, bad, everywhere, c.ref, c.hn, f"dense2 {fault}")
        changed = (bad != clean).nonzero()
        assert changed[:, 0].min() >= 16 and changed[:, 0].max() < 32 and changed[:, 1].min() >= 5 * 24 and changed[:, 1].max() < 6 * 24
    # the faults inside the GEMM stay under the rel-RMS bounds of the older comparisons (6e-3 against the separate launches,
    # 1.5e-2 against fp64)
    assert seen["kelem"][2] < 6e-3 and seen["kstep"][2] < 1.5e-2


def test_planted_faults_in_af_act_slabs_leave_the_tolerance():
    c = fo.slab_case(5, 4, 1, 768, 32, "cout", True, False, True)
    region = (slice(0, 1), slice(None), slice(0, 192))         # sample 0, the first workgroup's 8 groups
    _, clean, _ = fo.model_slabs(c, BF16)
    assert fo.check_elements(clean, c.ref, c.hn, BF16) <= 1.0
    for fault in ("slab_skipped", "pixswap", "temb_row", "group_stats", "gamma_beta", "residual_late"):
        _, bad, _ = fo.model_slabs(c, BF16, fault)
        _planted(clean, bad, region, c.ref, c.hn, f"af_act_slabs {fault}")
    # GroupNorm only (act = 0, what the attention block is handed) on 2x2 planes, nine slabs
    c = fo.slab_case(9, 2, 0, 192, 32, "wide", True, True, True)
    _, clean, _ = fo.model_slabs(c, BF16)
    for fault in ("slab_skipped", "pixswap", "temb_row", "group_stats", "gamma_beta", "residual_late"):
        _, bad, _ = fo.model_slabs(c, BF16, fault)
        _planted(clean, bad, region, c.ref, c.hn, f"af_act_slabs act 0 {fault}")


def test_planted_faults_in_y_norm_leave_the_tolerance():
    c = fo.ynorm_case(*fo.YNORM_CASES[0])
    region = (slice(0, 1), slice(None), slice(0, 96))          # sample 0, the first 96-cout tile
    _, clean = fo.model_ynorm(c)
    assert fo.check_elements(clean, c.hn, c.hn, BF16) <= 1.0
    for fault in ("pixswap", "group_stats", "gamma_beta"):
        _, bad = fo.model_ynorm(c, BF16, fault)
        _planted(clean, bad, region, c.hn, c.hn, f"y_norm {fault}")


def test_a_unit_fault_in_y_is_seen():
    """One element of y off by one (sigma <= 12: at least 1/12 of a normalised unit) puts elements outside the tolerance."""
    for row in fo.SLAB_CASES[:10]:
        c = fo.slab_case(*row)
        slabs = c.slabs.clone()
        slabs[0, 5, 7] += 1
        bad = fo.model_slabs(type("C", (), {**vars(c), "slabs": slabs}), BF16)[1]
        ratio = (bad.double().reshape(c.ref.shape) - c.ref).abs() / fo.tolerance(c.ref, c.hn, BF16)
        assert int((ratio > 1).sum()) >= 1, c.what


# ------------------------------------------------------------------------------------------------------------------ coverage guard
def _query(dt, B, H, C1, C2, Cout, KS, sc=None, defer=False, stats=False, G=0):
    """(workspace bytes, variant code, statistics splits, afldm_conv2d_norm_ok) of such a call, asked as ops.conv2d / conv2d_slabs
    ask (dummy 16-byte aligned addresses: the queries never dereference them)."""
    from afldm_amd import _lib
    lib, a, base = _lib.lib, _lib.ConvArgs(), 0x10000000
    a.x1, a.w, a.y = base, base + 16, base + 32
    a.x2 = base + 64 if C2 else None
    a.C1, a.C2, a.B, a.H, a.W, a.Cout, a.KS = C1, C2, B, H, H, Cout, KS
    a.y_ld, a.res_ld, a.dtype = Cout, Cout, _lib.DTYPE_CODE[dt]
    if not defer:
        a.bias = base + 48
    if sc is not None:
        a.sc_x1, a.sc_w, a.sc_C1, a.sc_C2 = base + 96, base + 128, sc[0], sc[1]
        a.sc_x2 = base + 112 if sc[1] else None
    if stats:
        a.stats_out = base + 160
    r = ctypes.byref(a)
    need = lib.afldm_conv2d_workspace(r)
    if need:
        a.workspace, a.workspace_bytes = base + 80, need
    a.defer_reduce = 1 if defer else 0
    code = lib.afldm_conv2d_variant(r)
    S = lib.afldm_conv2d_stats_splits(r) if stats else 0
    ok = 0
    if G:
        a.norm_gamma, a.norm_beta, a.norm_groups, a.norm_eps = base + 176, base + 192, G, 1e-5
        ok = lib.afldm_conv2d_norm_ok(r)
    return need, code, S, ok


def _nslab(dt, B, H, C1, C2, Cout, KS, sc=None):
    """Slices conv2d_slabs hands over for such a call, or 0 where it returns None."""
    need, code, _, _ = _query(dt, B, H, C1, C2, Cout, KS, sc, defer=True)
    n = (code >> 8) & 255 if code >= 0 else 1
    return 0 if (not need or code < 0 or n <= 1 or (code >> 16) & 1) else n


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_ffhq_site_of_the_three_launches_falls_in_a_class_the_gpu_file_runs(dtype):
    from afldm_amd import _lib
    B, G = 64, 32
    sites = unet_sites()
    seen = {"dense2": set(), "slabs": set(), "ynorm": set()}
    # 2^2 ResnetBlock2D sites: conv1 + temb -> norm2 -> activation in one launch
    for (H, C1, C2, Cout, KS) in sites:
        if H == 2 and KS == 3:
            assert _lib.lib.afldm_conv2x2_const_norm_act_supported(C1 + C2, Cout, G, _lib.DTYPE_CODE[dtype]), (C1, C2, Cout)
            cls = (dtype, Cout // G, (C1 + C2) // (fo.D2_WAVES * fo.kpf(dtype)))
            assert cls in DENSE2_CLASSES, f"2x2 site {C1}|{C2} -> {Cout}: class {cls} is compared with no reference"
            seen["dense2"].add(cls)
    # 4^2 sites: conv1 -> norm2 and conv2 (-> the attention block's norm) from their split-K slabs, the folded shortcut included;
    # the dense layers of the 2^2 level where they split K (conv2: [B, Cout] -> 4 Cout)
    shortcuts = [(C1, C2) for (H, C1, C2, Cout, KS) in sites if H == 4 and KS == 1 and Cout == 768 and C1 + C2 != Cout]
    # (conv1 reads the ONE tensor the first activation wrote for hidden | skip; at 2^2 conv1 is the fused launch above)
    calls = [(4, C1 + C2, 0, Cout, 3, None) for (H, C1, C2, Cout, KS) in sites if H == 4 and KS == 3]
    calls += [(4, 768, 0, 768, 3, sc) for sc in shortcuts]
    calls += [(1, Cout, 0, 4 * Cout, 1, None) for (H, C1, C2, Cout, KS) in sites if H == 2 and KS == 3]
    assert len(shortcuts) == 3 and len(calls) >= 9
    for (H, C1, C2, Cout, KS, sc) in calls:
        n = _nslab(dtype, B, H, C1, C2, Cout, KS, sc)
        if n:
            cls = (4 if H == 4 else 2, 768 // G, n)
            assert cls in SLAB_CLASSES, f"site {H} {C1}|{C2} -> {Cout} sc {sc}: class (N, cpg, nslab) = {cls} is compared with no reference"
            seen["slabs"].add(cls)
    assert any(c[0] == 4 for c in seen["slabs"]), "the 4x4 sites split K at batch 64"
    # 8^2 conv2 sites in front of attention (bf16): the epilogue applies the next norm where afldm_conv2d_norm_ok says so
    if dtype == BF16:
        for sc in (None, (768, 384), (384, 384)):
            need, code, S, ok = _query(dtype, B, 8, 384, 0, 384, 3, sc, stats=True, G=G)
            assert ok == 1 and not need and code & 255 == 51 and S == 1, (sc, need, code, S, ok)
            assert 384 // G in YNORM_CLASSES
            seen["ynorm"].add(384 // G)
    print(f"[fusednorm host] {dtype}: model classes at batch 64: {seen}")


def test_norm_ok_accepts_what_the_tables_say():
    """afldm_conv2d_norm_ok among Cin = Cout in {96, 192, 384, 768}, G in {8, 32} (bf16, 8^2 planes): NORM_OK_FROM holds the first
    batch it accepts, 768 is refused at 64, 96 always, fp32 always."""
    for Cout in (96, 192, 384, 768):
        for G in (8, 32):
            first = next((B for B in range(1, 65) if _query(BF16, B, 8, Cout, 0, Cout, 3, stats=True, G=G)[3]), None)
            assert first == fo.NORM_OK_FROM.get(Cout), (Cout, G, first)
            assert _query(BF16, 64, 8, Cout, 0, Cout, 3, stats=True, G=G)[3] == (1 if Cout in (192, 384) else 0)
            assert not _query(FP32, 64, 8, Cout, 0, Cout, 3, stats=True, G=G)[3]
    for (B, Cin, Cout, G, sc, _) in fo.YNORM_CASES:
        assert _query(BF16, B, 8, Cin, 0, Cout, 3, sc, stats=True, G=G)[3] == 1, (B, Cin, Cout, G, sc)
