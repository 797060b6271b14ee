"""GPU tests: the convolution / linear GEMM family bit for bit against a float64 evaluation on exact inputs (tests/exact_oracle.py).

Operands are small integers (activations and weights in {-1, 0, +1}; bias, time embedding and residual in [-8, 8]), so every
product and every partial sum is exact in fp32 in any order and the result is a bf16 value: the kernel must EQUAL the reference,
whatever its tiling, slicing or summation order, and the GroupNorm partial sums must equal the sums of the stored output.  There is
no tolerance anywhere in this file.  conv_out_fused (GroupNorm-apply and SiLU inside the launch) is covered on the inputs of
addressed_oracle.tail_case: dictated statistics with rstd = 1 and normalised values on which bf16(silu(v)) is v or 0.  Out of
scope (a GroupNorm-apply, SiLU, softmax or filter matrix inside the launch): act_conv_act, the trunk, the stand-alone af_* launches
and the attention kernels (tests/test_gpu_attention_addressed.py holds the fused attention block to a derived per-element tolerance
instead).  dense2.hip, afldm_af_act_slabs and the y_norm epilogue normalise the convolution's own output: on integer operands that
output and its statistics are exact, and tests/test_gpu_fused_norm_exact.py holds what follows to a half-ulp tolerance per element
(y_norm here too: test_norm_out_*).
"""
import ctypes
import functools

import pytest
import torch

import addressed_oracle as ado
import exact_oracle as xo
import fusednorm_oracle as fo
from exact_oracle import assert_exact, assert_stats_exact, conv_case

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = [FP32, BF16]
DT = {"bf16": BF16, "fp32": FP32}


def _ops():
    from afldm_amd import ops
    return ops


def _lib():
    from afldm_amd import _lib
    return _lib


def dev(t, dtype):
    return None if t is None else t.to(dtype).cuda().contiguous()


def operands(c, dtype):
    """The case's tensors on the GPU in `dtype` (bias stays fp32, as every caller passes it); per-sample weights: sample 0's
    tensor of the contiguous stack + the stride between samples."""
    o = dict(x1=dev(c.x1, dtype), x2=dev(c.x2, dtype), w=dev(c.w, dtype), bias=dev(c.bias, FP32), temb=dev(c.temb, dtype),
             residual=dev(c.residual, dtype), shortcut=None, w_batch_stride=0)
    if c.shortcut is not None:
        o["shortcut"] = tuple(dev(t, dtype) for t in c.shortcut)
    if c.per_sample_w:
        o["w_all"], o["w"] = o["w"], o["w"][0]
        o["w_batch_stride"] = o["w"].numel()
    return o


def conv_kwargs(c, o):
    kw = dict(x2=o["x2"], temb=o["temb"], temb_stride=0 if o["temb"] is None else o["temb"].shape[1], residual=o["residual"],
              temb_mod=c.temb_mod)
    if o["shortcut"] is not None:
        kw["shortcut"] = o["shortcut"]
    if o["w_batch_stride"]:
        kw["w_batch_stride"] = o["w_batch_stride"]
    return kw


def run_exact(c, dtype, want_stats=True, what="", **extra):
    """ops.conv2d on the case, compared with its float64 reference (and its statistics with the stored output)."""
    ops = _ops()
    o = operands(c, dtype)
    want_stats = want_stats and c.Cout % 4 == 0 and not c.per_sample_w
    y = ops.conv2d(o["x1"], o["w"], o["bias"], want_stats=want_stats, **conv_kwargs(c, o), **extra)
    assert_exact(y, c.ref, f"{what} {c.what} {dtype}")
    if want_stats:
        assert_stats_exact(y.gn_partial, y, f"{what} {c.what} {dtype}")
    return y, o


def variant_code(c, o, y, workspace=None):
    """afldm_conv2d_variant of the call run_exact makes: variant | splitk << 8 | fused << 16 (negative: not the GEMM path)."""
    ops, L = _ops(), _lib()
    kw = conv_kwargs(c, o)
    a = ops.conv_args(o["x1"], o["w"], o["bias"], kw["x2"], kw["temb"], kw["temb_stride"], kw["residual"], y, temb_mod=c.temb_mod)
    if workspace is None:
        need = L.lib.afldm_conv2d_workspace(ctypes.byref(a))
        workspace = torch.empty(max(need, 4) // 4, dtype=FP32, device="cuda")
        a.workspace, a.workspace_bytes = L.ptr(workspace), need
    else:
        a.workspace, a.workspace_bytes = L.ptr(workspace), workspace.numel() * 4
    return L.lib.afldm_conv2d_variant(ctypes.byref(a))


class Failures:
    """Collects the mismatches of a loop over many sub-cases, so that one run names every failing one."""

    def __init__(self):
        self.msgs = []

    def run(self, what, fn):
        try:
            fn()
        except AssertionError as e:           # (anything else - a launch error - ends the test at once)
            self.msgs.append(f"[{what}] {type(e).__name__}: {str(e)[:600]}")

    def check(self):
        assert not self.msgs, f"{len(self.msgs)} sub-cases failed:\n" + "\n".join(self.msgs)


def _nhwc_to_c8(t):
    B, N, _, C = t.shape
    out = t.reshape(B, N, N, C // 8, 8).permute(0, 3, 1, 2, 4).contiguous().view(B, N, N, C)
    out.c8 = True
    return out


def _c8_to_nhwc(t):
    B, N, _, C = t.shape
    return t.reshape(B, C // 8, N, N, 8).permute(0, 2, 3, 1, 4).reshape(B, N, N, C)


# ================================================================================================ a. the planner's own choice
_SITES = {}


def _record(model, dtype):
    """The distinct ops.conv2d / conv2d_s2 / conv2d_up2 / linear_split calls of one forward at batch 1 with random weights: the
    FFHQ-config UNet or the AF-VAE decoder.  A site is the call's shapes and keyword set."""
    key = (model, dtype)
    if key in _SITES:
        return _SITES[key]
    ops = _ops()
    from test_gpu_r02 import build_full_vae, build_unet
    sites = {}
    real = {n: getattr(ops, n) for n in ("conv2d", "conv2d_s2", "conv2d_up2", "linear_split")}

    def conv2d(x1, w, bias=None, x2=None, temb=None, temb_stride=0, residual=None, out=None, out_mode=0, workspace=None,
               want_stats=False, temb_mod=0, w_batch_stride=0, norm_out=None, out_c8=False, shortcut=None):
        sc = None if shortcut is None else (shortcut[0].shape[-1], 0 if shortcut[1] is None else shortcut[1].shape[-1])
        site = ("conv2d", tuple(x1.shape), 0 if x2 is None else x2.shape[-1], w.shape[0], w.shape[1], temb is not None, int(temb_mod),
                residual is not None, bool(want_stats), sc, int(out_mode), bool(ops.is_c8(x1)), bool(out_c8), norm_out is not None,
                w_batch_stride != 0, bias is not None)
        sites.setdefault(site, len(sites))
        return real["conv2d"](x1, w, bias, x2=x2, temb=temb, temb_stride=temb_stride, residual=residual, out=out, out_mode=out_mode,
                              workspace=workspace, want_stats=want_stats, temb_mod=temb_mod, w_batch_stride=w_batch_stride,
                              norm_out=norm_out, out_c8=out_c8, shortcut=shortcut)

    def conv2d_s2(x, w, bias=None, pad=(1, 1), want_stats=False, out=None):
        sites.setdefault(("s2", tuple(x.shape), w.shape[0], tuple(pad), bool(want_stats)), len(sites))
        return real["conv2d_s2"](x, w, bias, pad=pad, want_stats=want_stats, out=out)

    def conv2d_up2(x, w_up2, bias=None, want_stats=False, out=None):
        sites.setdefault(("up2", tuple(x.shape), w_up2.shape[1], bool(want_stats)), len(sites))
        return real["conv2d_up2"](x, w_up2, bias, want_stats=want_stats, out=out)

    def linear_split(x, w, bias, split_n, workspace=None):
        sites.setdefault(("split", tuple(x.shape), w.shape[0], int(split_n)), len(sites))
        return real["linear_split"](x, w, bias, split_n, workspace=workspace)

    g = torch.Generator().manual_seed(3)
    try:
        for n, f in (("conv2d", conv2d), ("conv2d_s2", conv2d_s2), ("conv2d_up2", conv2d_up2), ("linear_split", linear_split)):
            setattr(ops, n, f)
        with torch.no_grad():
            if model == "unet":
                net, cfg, _ = build_unet("ffhq", dtype)
                x = torch.randn(1, cfg["in_channels"], cfg["sample_size"], cfg["sample_size"], generator=g).cuda().to(dtype)
                net(x, 981)
            else:
                net, _, _ = build_full_vae(dtype)
                net.decode(torch.randn(1, 4, 32, 32, generator=g).cuda().to(dtype), return_dict=False)
        torch.cuda.synchronize()
    finally:
        for n, f in real.items():
            setattr(ops, n, f)
    del net
    _SITES[key] = sorted(sites, key=sites.get)
    return _SITES[key]


def _site_batches(HW, big):
    """B = 1 and 3; 8 where tiles hold several samples (8^2, 4^2 planes); 40 on 2^2 planes (16 samples per tile, ragged last
    tile); planes above 64^2 run as one 64 x 96 crop."""
    if big:
        return (1,)
    return (1, 3) + ((8,) if HW in (64, 16) else ()) + ((40,) if HW == 4 else ())


def _run_conv2d_site(site, dtype, fails):
    ops = _ops()
    _, shape, C2, Cout, KS, temb, temb_mod, res, stats, sc, out_mode, c8, out_c8, norm, wB, has_bias = site
    C1 = shape[-1]
    if len(shape) == 4:
        H, W = shape[1], shape[2]
        big = H * W > 64 * 64
        if big:
            H, W = 64, 96
        batches = _site_batches(H * W, big)
    elif len(shape) == 3:
        H, W, batches = shape[1], 1, (1, 3)
    else:
        H, W, batches = 1, 1, (1, 3, 40, 64)     # a linear layer over rows (the time MLP, the dense form of the 2^2 level): M = 1 .. 64
    for B in batches:
        def one(B=B):
            c = conv_case(B, H, W, C1, C2, Cout, KS, temb=temb, temb_mod=temb_mod, residual=res and sc is None, shortcut=sc,
                          per_sample_w=wB, bias=has_bias)
            o = operands(c, dtype)
            view = (lambda t: t) if len(shape) == 4 else (lambda t: None if t is None else t.reshape((B,) + (() if len(shape) == 2 else (H,)) + (t.shape[-1],)))
            x1, x2, resid = view(o["x1"]), view(o["x2"]), view(o["residual"])
            kw = dict(x2=x2, temb=o["temb"], temb_stride=0 if o["temb"] is None else o["temb"].shape[1], residual=resid,
                      temb_mod=temb_mod, out_mode=out_mode, want_stats=stats)
            if wB:
                kw["w_batch_stride"] = o["w_batch_stride"]
            if norm:
                kw["norm_out"] = (torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda"), 32, 1e-5)
            use_c8 = (c8 or out_c8) and ops.conv2d_c8_ok(o["x1"], o["w"], o["bias"], temb=o["temb"], temb_stride=kw["temb_stride"],
                                                         residual=resid, want_stats=stats)
            if use_c8 and c8:
                x1 = _nhwc_to_c8(x1)
            if use_c8 and out_c8:
                kw["out_c8"] = True
            if sc is not None and ops.conv2d_shortcut_ok(o["x1"], o["w"], o["bias"], o["shortcut"], temb=o["temb"],
                                                         temb_stride=kw["temb_stride"], want_stats=stats):
                kw["shortcut"] = o["shortcut"]
            elif sc is not None:             # the block's own route where the fold is not available: the 1x1 launch, then the 3x3
                kw["residual"] = ops.conv2d(o["shortcut"][0], o["shortcut"][2], None, x2=o["shortcut"][1])
            try:
                y = ops.conv2d(x1, o["w"], o["bias"], **kw)
            except RuntimeError as e:
                if not (wB and "w_batch_stride" in str(e)):
                    raise
                # attention_dense's own route where one launch cannot take per-sample weights: a launch per sample
                kw.pop("w_batch_stride")
                y = torch.cat([ops.conv2d(x1[b:b + 1].contiguous(), o["w_all"][b], o["bias"], **kw) for b in range(B)], 0)
            got = _c8_to_nhwc(y) if kw.get("out_c8") else y
            if out_mode == 1:
                got = got.transpose(1, 2)
            assert_exact(got.reshape(c.ref.shape), c.ref, c.what)
            if getattr(y, "gn_partial", None) is not None:
                assert_stats_exact(y.gn_partial, got.reshape(y.gn_partial.shape[0], -1, Cout), c.what)
        fails.run(f"{site} B={B}", one)


def _run_other_site(site, dtype, fails):
    ops = _ops()
    kind, shape = site[0], site[1]
    if kind == "split":
        _, _, Cout, split_n = site
        for B in (1, 3):
            fails.run(f"{site} B={B}", lambda B=B: _linear_split_exact(B, shape[1], shape[2], Cout, split_n, dtype))
        return
    H, W = shape[1], shape[2]
    big = H * W > 64 * 64
    if big:
        H, W = 64, 96
    for B in _site_batches(H * W, big):
        def one(B=B):
            c = xo.resample_case(kind, site[3] if kind == "s2" else None, B, H, W, shape[3], site[2])
            _resample_exact(c, dtype, want_stats=site[-1])
        fails.run(f"{site} B={B}", one)


PARTS = 4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("model", ["unet", "vae"])
def test_model_sites_planner_choice(model, part, dtype):
    """Every distinct GEMM call site of one FFHQ-config UNet forward / one AF-VAE decoder forward, as the planner runs it (nothing
    forced), with the call's keyword set, at B = 1 and 3, B = 8 on 8^2 / 4^2 planes, B = 40 on 2^2 planes, linear layers over
    rows at M = 1, 3, 40 and 64; VAE planes above 64^2 as a 64 x 96 crop with the site's channel counts.  A site runs with one
    time embedding row per sample where the forward shares one row.  Where the model itself asks before it folds the shortcut
    or uses the 8-channel-block layout, so does the case.  Convolutions that the forward runs inside a merged launch
    (act_conv_act, the trunk, conv_out_fused) are not ops.conv2d calls and are out of scope here; their shapes are in the
    forced-variant and plumbing tests below.  (The sites are split into parts to keep each test short.)"""
    sites = _record(model, dtype)
    assert sites, "the forward recorded no GEMM call"
    if model == "unet":
        assert any(s[0] == "conv2d" and len(s[1]) == 4 and s[4] == 3 for s in sites), "no 3x3 convolution recorded"
    if part == 0:
        print(f"[exact] {model} {dtype}: {len(sites)} distinct sites")
        for s in sites:
            print("[exact]   ", s)
    fails = Failures()
    for s in sites[part::PARTS]:
        (_run_conv2d_site if s[0] == "conv2d" else _run_other_site)(s, dtype, fails)
    fails.check()


# ================================================================================================ b. every variant
# the ids afldm_conv2d_tune accepts (sparse: retired tuning variants are refused), and the general GEMM tiles among them
LIVE_CONV_VARIANTS = [0, 1, 3, 29, 30, 31, 32, 33, 41, 43, 46, 51, 52, 54, 55, 58, 63, 65, 66, 67, 68]
GENERAL_GEMM_VARIANTS = [0, 1, 3, 29, 30, 31, 32, 33]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_gemm_variant_exact(dtype):
    """The loop of test_conv2d_every_gemm_variant on its ragged shape (2 x 12 x 12, 128 | 64 -> 200, residual), split-K 1 and 3:
    every variant afldm_conv2d_tune accepts among ids 0 ... 68 - exactly the live list.  The halo-patch variants (41 and up) cannot
    take the shape and fall back (as there; they have their own tests below); the general GEMM tiles (0, 1, 3, 29 - 33) must be the
    ones that ran."""
    ops, L = _ops(), _lib()
    c = conv_case(**xo.EVERY_VARIANT)
    o = operands(c, dtype)
    ws = torch.empty(4 * c.B * c.H * c.W * c.Cout, dtype=FP32, device="cuda")
    fails, accepted, ran = Failures(), [], set()
    try:
        for v in range(69):
            if L.lib.afldm_conv2d_tune(v, 1) != 0:
                continue                  # a retired id: refused, the forcing stays as it was
            accepted.append(v)
            for sk in (1, 3):
                L.check(L.lib.afldm_conv2d_tune(v, sk), "tune")

                def one():
                    y = ops.conv2d(o["x1"], o["w"], o["bias"], x2=o["x2"], residual=o["residual"], workspace=ws)
                    code = variant_code(c, o, y, ws)
                    if code >= 0 and code & 255 == v:
                        ran.add((v, (code >> 8) & 255))
                    assert_exact(y, c.ref, f"variant {v} split-K {sk} (ran {code & 255 if code >= 0 else code})")
                fails.run(f"variant {v} split-K {sk}", one)
    finally:
        L.lib.afldm_conv2d_tune(-1, -1)
    fails.check()
    assert accepted == LIVE_CONV_VARIANTS
    print(f"[exact] variants that took the ragged shape ({dtype}): {sorted(ran)}")
    want = {(v, z) for v in GENERAL_GEMM_VARIANTS for z in (1, 3)}      # every general GEMM tile takes any shape, with 1 and 3 slices
    assert ran >= want, sorted(want - ran)


def _forced(c, dtype, v, sk=-1, stats=True):
    """conv2d with the variant forced; asserts it ran and the result is exact.  Returns (y, code)."""
    L = _lib()
    try:
        L.check(L.lib.afldm_conv2d_tune(v, sk), "tune")
        y, o = run_exact(c, dtype, want_stats=stats, what=f"variant {v}")
        code = variant_code(c, o, y)           # (with the workspace the forced plan asks for, as ops.conv2d gave it)
        assert code >= 0 and code & 255 == v, f"variant {v} did not run {c.what} (code {code})"
    finally:
        L.lib.afldm_conv2d_tune(-1, -1)
    return y, code


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(xo.H3_EXACT)))
def test_halo_patch_variants_exact(dtype, i):
    """conv3h.hip variants on the H3_CASES shapes (batches cut to what fills two tiles), forced and checked to have run."""
    kw, variants = xo.H3_EXACT[i]
    c = conv_case(**kw)
    fails = Failures()
    for v in variants:
        fails.run(f"variant {v}", lambda v=v: _forced(c, dtype, v))
    fails.check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(xo.V58_EXACT)))
def test_halo_patch_on_blocks_of_large_planes_exact(dtype, i):
    """Variant 58: 8 x 32 pixel blocks of a plane larger than a tile, one of them non-square (72 x 96)."""
    _forced(conv_case(**xo.V58_EXACT[i]), dtype, 58)


# ================================================================================================ c. split-K
def _splitk_launch(c, o, fused, stats=True):
    """One afldm_conv2d with a workspace for up to 8 slices, with (fused) or without the sync words; -> (y, statistics, code)."""
    ops, L = _ops(), _lib()
    kw = conv_kwargs(c, o)
    y = torch.empty(c.B, c.H, c.W, c.Cout, dtype=o["x1"].dtype, device="cuda")
    a = ops.conv_args(o["x1"], o["w"], o["bias"], temb=kw["temb"], temb_stride=kw["temb_stride"], residual=kw["residual"], out=y)
    if not fused:
        a.sync, a.sync_bytes = None, 0
    ws = torch.empty(8 * c.B * c.H * c.W * c.Cout, dtype=FP32, device="cuda")
    a.workspace, a.workspace_bytes = L.ptr(ws), ws.numel() * 4
    code = L.lib.afldm_conv2d_variant(ctypes.byref(a))
    S = L.lib.afldm_conv2d_stats_splits(ctypes.byref(a))
    st = torch.zeros(c.B, S, c.Cout, 2, dtype=FP32, device="cuda")
    a.stats_out = L.ptr(st)
    ops.conv2d_launch(a)
    return y, st, code


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(xo.SPLITK_EXACT)))
def test_split_k_exact(dtype, i):
    """The three forms of a split-K convolution at the 4^2, 8^2 and M = 48 shapes: slabs + the reduction launch, the reduction
    inside the launch (afldm_conv2d_fused_splitk; no slice timed out, the counter words are zero again), and the slabs handed
    over (conv2d_slabs), whose float64 sum is the convolution without bias, time embedding and residual.  The planner's own
    choice, 2 / 4 slices forced on it, and 2 / 4 slices on the 128 x 192 and 64 x 64 LDS-DMA tiles (variants 29, 32: the ones that
    can reduce inside the launch).  The slabs are fp32: no rounding before the store."""
    ops, L = _ops(), _lib()
    c = conv_case(**xo.SPLITK_EXACT[i])
    o = operands(c, dtype)
    plain = xo.reference(c, plain=True)
    fails, seen = Failures(), {"two": set(), "fused": set(), "slabs": set()}
    try:
        for v, sk in ((-1, -1), (-1, 2), (-1, 4), (29, 2), (29, 4), (32, 2), (32, 4)):
            L.check(L.lib.afldm_conv2d_tune(v, sk), "tune")

            def two():
                y, st, code = _splitk_launch(c, o, fused=False)
                assert code >= 0 and not (code >> 16) & 1
                seen["two"].add((code >> 8) & 255)
                assert_exact(y, c.ref, f"two launches, variant {v} split-K {sk} (code {code:#x})")
                assert_stats_exact(st, y, f"two launches, variant {v} split-K {sk}")
            fails.run(f"two launches {v}/{sk}", two)

            def fused():
                L.check(L.lib.afldm_conv2d_fused_splitk(1), "fused_splitk")
                try:
                    y, st, code = _splitk_launch(c, o, fused=True)
                    torch.cuda.synchronize()
                finally:
                    L.lib.afldm_conv2d_fused_splitk(0)
                if (code >> 16) & 1:
                    seen["fused"].add((code >> 8) & 255)
                assert not ops.fused_splitk_error(), "a slice timed out"
                assert int(ops._sync_words(o["x1"].device).abs().sum()) == 0, "counter words left non-zero"
                assert_exact(y, c.ref, f"fused reduction, variant {v} split-K {sk} (code {code:#x})")
                assert_stats_exact(st, y, f"fused reduction, variant {v} split-K {sk}")
            fails.run(f"fused {v}/{sk}", fused)

            def slabs():
                got = ops.conv2d_slabs(o["x1"], o["w"])
                if got is None:
                    return
                s, n = got
                seen["slabs"].add(n)
                assert_exact(s.double().sum(0).view(plain.shape), plain, f"sum of {n} slabs, variant {v} split-K {sk}")
            fails.run(f"slabs {v}/{sk}", slabs)
    finally:
        L.lib.afldm_conv2d_tune(-1, -1)
        L.lib.afldm_conv2d_fused_splitk(0)
    fails.check()
    print(f"[exact] split-K slice counts seen {c.what} {dtype}: {seen}")
    assert any(z > 1 for z in seen["two"]), seen
    assert seen["fused"], "no launch reduced its slices itself"
    assert seen["slabs"], "conv2d_slabs never handed slabs over"


# ================================================================================================ d. the folded shortcut
def shortcut_kind(o, want_stats=True):
    """afldm_conv2d_shortcut_ok of the folded call under the tuning in force now, asked as ops.conv2d_shortcut_ok asks it but
    without that function's cache (its key does not carry afldm_conv2d_tune): 0 none, 1 one tap per K step, 2 three taps."""
    ops, L = _ops(), _lib()
    sc = o["shortcut"]
    a = ops.conv_args(o["x1"], o["w"], o["bias"], None, o["temb"], 0 if o["temb"] is None else o["temb"].shape[1], None, None)
    a.y = L.ptr(sc[0])                    # (a non-NULL, aligned placeholder: the queries do not dereference it)
    if want_stats and o["w"].shape[0] % 4 == 0:
        a.stats_out = L.ptr(sc[0])
    ops._set_shortcut(a, sc)
    need = L.lib.afldm_conv2d_workspace(ctypes.byref(a))
    if need:
        a.workspace, a.workspace_bytes = L.ptr(sc[0]), need
    return int(L.lib.afldm_conv2d_shortcut_ok(ctypes.byref(a))), L.lib.afldm_conv2d_variant(ctypes.byref(a))


def _fold_exact(N, C1, C2, Cout, B, dtype, kind, force=None):
    """conv3x3(h) + conv1x1(x1 | x2): the folded call - which must exist, on a tile of the expected kind (and, forced, of that
    variant) - the two launches it replaces and the float64 reference, all equal.  The two-launch form stores the 1x1 output in
    `dtype` before the 3x3 adds it: at most K_sc * density products of +-1 plus the bias, an integer far inside +-256
    (K_sc <= 1536, density <= 0.5 * 0.5: sigma <= 20), so that store is exact too."""
    ops, L = _ops(), _lib()
    c = xo.fold_case(N, C1, C2, Cout, B)
    o = operands(c, dtype)
    sc = o["shortcut"]
    bsc = xo.small_ints((Cout,), -4, 4, torch.Generator().manual_seed(C1 + B))
    b2 = dev(c.bias - bsc, FP32)
    res = ops.conv2d(sc[0], sc[2], dev(bsc, FP32), x2=sc[1])
    assert float(res.float().abs().max()) <= xo.MAX_ABS
    two = ops.conv2d(o["x1"], o["w"], b2, residual=res, want_stats=True)
    what = f"{c.what} {dtype}" + (f" variant {force}" if force is not None else "")
    assert_exact(two, c.ref, "two launches " + what)
    assert_stats_exact(two.gn_partial, two, "two launches " + what)
    try:
        if force is not None:
            L.check(L.lib.afldm_conv2d_tune(force, 1), "tune")
        ok, code = shortcut_kind(o)
        assert ok == kind, f"{what}: afldm_conv2d_shortcut_ok gives {ok} (variant code {code:#x}), the case expects {kind}"
        if force is None:
            assert ops.conv2d_shortcut_ok(o["x1"], o["w"], o["bias"], sc) == kind
        else:
            assert code >= 0 and code & 255 == force, f"variant {force} did not take {what} (code {code:#x})"
        got = ops.conv2d(o["x1"], o["w"], o["bias"], want_stats=True, shortcut=sc)
    finally:
        L.lib.afldm_conv2d_tune(-1, -1)
    assert_exact(got, c.ref, "folded " + what)
    assert_stats_exact(got.gn_partial, got, "folded " + what)
    assert torch.equal(got, two)
    return o["x1"], o["w"]


@pytest.mark.parametrize("N,C1,C2,Cout,B,dt,kind,force", xo.FOLD_CASES)
def test_shortcut_fold_exact(N, C1, C2, Cout, B, dt, kind, force):
    """Every case makes a folded call on a tile of the stated kind (exact_oracle.FOLD_CASES): the three-tap fold of the 8^2 / 4^2
    sites at batch 64 (both dtypes) and on the bf16 small-batch tiles of every site; the one-tap fold of the 16^2 / 32^2 sites
    at batch 64 (both dtypes: what the benchmark runs) and, forced, on variants 41 / 46 / 43 at B = 1 / 2."""
    _fold_exact(N, C1, C2, Cout, B, DT[dt], kind, force)


@pytest.mark.parametrize("dt,C1,C2,what", xo.FOLD_SHARES)
def test_shortcut_fold_splitk_shares_exact(dt, C1, C2, what):
    """The split-K share cases of test_conv2d_shortcut_fold3_splitk_shares (4^2 planes, batch 64, 384 couts): slices whose shares
    of the shortcut's channel blocks differ, and an sc_x1 | sc_x2 boundary that falls between two slices."""
    from test_gpu_shortcut_fold3 import _splitk
    dtype = DT[dt]
    got = _fold_exact(4, C1, C2, 384, 64, dtype, 2)
    z = _splitk(*got)
    kstep = 128 // got[0].element_size()
    nsc, nb1 = (C1 + C2) // kstep, C1 // kstep
    edges = [nsc * k // z for k in range(z + 1)]
    shares = [b - a for a, b in zip(edges, edges[1:])]
    assert z > 1, z
    if what == "uneven":
        assert len(set(shares)) > 1, (z, shares)
    else:
        assert nb1 in edges[1:-1], (z, edges, nb1)


# ================================================================================================ e. operand plumbing
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(xo.SEAM_EXACT)))
def test_concat_seam_exact(dtype, i):
    """x1 | x2 at every C1 the FFHQ UNet concatenates at, and at the smallest the GEMM path takes: one K step, 64 bf16 / 32 fp32
    channels (32 | 32 runs in fp32 only: in bf16 a K step would straddle the seam and afldm_conv2d refuses the shape)."""
    kw = xo.SEAM_EXACT[i]
    if dtype == BF16 and kw["C1"] % 64:
        ops = _ops()
        c = conv_case(**kw)
        o = operands(c, dtype)
        with pytest.raises(RuntimeError, match="Cin"):
            ops.conv2d(o["x1"], o["w"], o["bias"], x2=o["x2"])
        return
    run_exact(conv_case(**kw), dtype, what="seam")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C1,C2,Co", [(5, 256, 0, 64), (16, 384, 128, 96), (64, 3072, 0, 768)])
def test_temb_mod_exact(dtype, B, C1, C2, Co):
    """temb_mod: channel n of the 4 Co outputs takes column n % Co of the time embedding (the dense form of the 2^2 level)."""
    run_exact(conv_case(B, 1, 1, C1, C2, 4 * Co, 1, temb=True, temb_mod=Co, residual=True), dtype, what="temb_mod")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [16, 64, 128])
def test_per_sample_weights_exact(dtype, T):
    """w_batch_stride as attention_dense uses it: scores q K^T (x [B, T, 1, C], sample b's K_b [T, C] its weights) and P V^T
    (x [B, T, 1, T], V_b^T [C, T]) on integer operands.  Where one launch cannot take per-sample weights (a tile that straddles
    samples, a reduction shorter than a K step) the call raises naming w_batch_stride and attention_dense runs a launch per
    sample: so does the case."""
    ops = _ops()
    B, C = 3, 64
    for what, Cin, Cout in (("scores", C, T), ("P V^T", T, C)):
        c = conv_case(B, T, 1, Cin, 0, Cout, 1, per_sample_w=True, bias=False)
        o = operands(c, dtype)
        try:
            y = ops.conv2d(o["x1"], o["w"], None, w_batch_stride=o["w_batch_stride"])
            route = "one launch"
        except RuntimeError as e:
            assert "w_batch_stride" in str(e), e
            y = torch.cat([ops.conv2d(o["x1"][b:b + 1].contiguous(), o["w_all"][b]) for b in range(B)], 0)
            route = "per sample"
        print(f"[exact] per-sample weights {what} T={T} {dtype}: {route}")
        assert_exact(y, c.ref, f"{what} T={T} ({route})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C,Cout", [(2, 8, 8, 64, 96), (3, 5, 7, 64, 40), (2, 32, 32, 192, 192)])
def test_channel_major_output_exact(dtype, B, H, W, C, Cout):
    """out_mode = 1: the [B, Cout, H * W] output (V^T), pixel counts that are and are not whole 16-byte runs."""
    ops = _ops()
    c = conv_case(B, H, W, C, 0, Cout, 1)
    o = operands(c, dtype)
    yt = ops.conv2d(o["x1"], o["w"], o["bias"], out_mode=1)
    assert yt.shape == (B, Cout, H * W)
    assert_exact(yt.transpose(1, 2).reshape(c.ref.shape), c.ref, c.what + " out_mode 1")


def _linear_split_exact(B, T, C, Cout, split_n, dtype):
    ops = _ops()
    c = conv_case(B, T, 1, C, 0, Cout, 1)
    o = operands(c, dtype)
    y, y2 = ops.linear_split(o["x1"].view(B, T, C), o["w"], o["bias"], split_n)
    ref = c.ref.view(B, T, Cout)
    assert_exact(y, ref[..., :split_n].contiguous(), c.what + " token-major rows")
    assert_exact(y2.transpose(1, 2), ref[..., split_n:].contiguous(), c.what + " channel-major rows")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,C", [(3, 100, 192), (1, 1040, 384), (4, 1024, 192), (16, 256, 384)])
def test_linear_split_exact(dtype, B, T, C):
    """linear_split (q | k token-major, v channel-major), both outputs: M = 300 and 1040 are no multiple of the token tile (the
    general kernel); M = 4096 at K = 192 / 384 with 1024 / 256 tokens per sample meets every condition of lin.hip's
    weights-in-registers kernel in bf16 (lin_wreg_bm: K in {192, 384}, M >= 4096, M and H W multiples of 32, H W > 64, split_n
    and Cout multiples of its N tile).  No host query reports that kernel - afldm_conv2d_variant names the GEMM tile the call
    would otherwise take - so which of the two ran is not asserted here; test_weights_in_registers_projections shows they are
    bit-identical, and both are held to the float64 reference by the cases of this test."""
    _linear_split_exact(B, T, C, 3 * C, 2 * C, dtype)


@pytest.mark.parametrize("C,B,HW", [(192, 4, 1024), (384, 16, 256)])
def test_attention_to_out_exact(C, B, HW):
    """to_out at the attention sizes (bf16, M = 4096, K = 192 / 384) with residual and statistics: lin.hip leaves these to the
    general GEMM tiles (its kernel takes the fused q | k | v projection only), statistics from their epilogue."""
    side = int(round(HW ** 0.5))
    c = conv_case(B, side, side, C, 0, C, 1, residual=True)
    y, o = run_exact(c, BF16, what="to_out")
    assert variant_code(c, o, y) >= 0, "to_out runs on the GEMM path"


# (plane, Cin, Cout, B, tile): the tile that must take the c8 call - the batch-64 halo-patch tiles (41 at 32^2, 43 at 16^2: what the
# benchmark runs) and the 64-pixel small-batch tiles (65 / 66) - or None where the plan splits K (batch 2; 384 -> 384 at 16^2 up to
# batch 8): conv2d_c8_ok must then say no and the call must be refused
C8_CASES = [(32, 192, 192, 2, None), (32, 192, 192, 8, 65), (32, 192, 192, 64, 41),
            (16, 384, 384, 2, None), (16, 384, 384, 8, None), (16, 384, 384, 64, 43),
            (32, 384, 192, 2, None), (32, 384, 192, 8, 65), (32, 384, 192, 64, 41),
            (16, 192, 384, 2, None), (16, 192, 384, 8, 66), (16, 192, 384, 64, 43)]


@pytest.mark.parametrize("N,C,Cout,B,tile", C8_CASES)
def test_c8_layout_exact(N, C, Cout, B, tile):
    """8-channel-block operands (bf16, 16^2 / 32^2): c8 in -> c8 out with time embedding and statistics, c8 in -> NHWC out with a
    residual.  conv2d_c8_ok must say yes for both and the stated tile must be the one that ran; where the case expects no c8
    convolution, conv2d_c8_ok must say no and afldm_conv2d must refuse the layout."""
    ops = _ops()
    c = conv_case(B, N, N, C, 0, Cout, 3, temb=True)
    o = operands(c, BF16)
    ok = ops.conv2d_c8_ok(o["x1"], o["w"], o["bias"], temb=o["temb"], temb_stride=Cout)
    assert ok == (tile is not None), f"conv2d_c8_ok gives {ok} for {c.what}"
    if tile is None:
        with pytest.raises(RuntimeError, match="8-channel blocks"):
            ops.conv2d(_nhwc_to_c8(o["x1"]), o["w"], o["bias"], temb=o["temb"], temb_stride=Cout, want_stats=True, out_c8=True)
        return
    y = ops.conv2d(_nhwc_to_c8(o["x1"]), o["w"], o["bias"], temb=o["temb"], temb_stride=Cout, want_stats=True, out_c8=True)
    code = variant_code(c, o, y)
    assert code >= 0 and code & 255 == tile and (code >> 8) & 255 == 1, f"{c.what}: ran {code:#x}"
    assert ops.is_c8(y)
    assert_exact(_c8_to_nhwc(y), c.ref, c.what + " c8 -> c8")
    assert_stats_exact(y.gn_partial, _c8_to_nhwc(y), c.what + " c8 -> c8")
    c2 = conv_case(B, N, N, C, 0, Cout, 3, residual=True, seed=1)
    o2 = operands(c2, BF16)
    assert ops.conv2d_c8_ok(o2["x1"], o2["w"], o2["bias"], residual=o2["residual"]), "no c8 -> NHWC convolution for " + c2.what
    y2 = ops.conv2d(_nhwc_to_c8(o2["x1"]), o2["w"], o2["bias"], residual=o2["residual"], want_stats=True)
    code = variant_code(c2, o2, y2)
    assert code >= 0 and code & 255 == tile, f"{c2.what}: ran {code:#x}"
    assert not ops.is_c8(y2)
    assert_exact(y2, c2.ref, c2.what + " c8 -> NHWC")
    assert_stats_exact(y2.gn_partial, y2, c2.what + " c8 -> NHWC")


@functools.lru_cache(None)
def _norm_out_case(B, C, Cout, sc):
    return conv_case(B, 8, 8, C, 0, Cout, 3, temb=sc is None, shortcut=sc)


def _norm_out(B, C, Cout, G, sc, applied):
    """conv2d with norm_out = per-channel (gamma in [0.5, 1.5], beta ~ 0.3 N(0, 1)), G groups: y and its statistics exact; where the
    epilogue normalised (`applied`), y.norm_applied within fusednorm_oracle.check_elements of float64 GroupNorm of the exact y."""
    ops = _ops()
    c = _norm_out_case(B, C, Cout, sc)
    o = operands(c, BF16)
    kw = conv_kwargs(c, o)
    if sc is not None:
        assert ops.conv2d_shortcut_ok(o["x1"], o["w"], o["bias"], o["shortcut"]) == 2
    gen = torch.Generator().manual_seed(Cout + G)
    gamma, beta = (torch.rand(Cout, generator=gen) + 0.5).float(), (torch.randn(Cout, generator=gen) * 0.3).float()
    y = ops.conv2d(o["x1"], o["w"], o["bias"], want_stats=True, norm_out=(gamma.cuda(), beta.cuda(), G, fo.EPS), **kw)
    hn = getattr(y, "norm_applied", None)
    if applied:
        assert hn is not None, "the one-sample 8x8 tile normalises in its epilogue"
    assert_exact(y, c.ref, c.what + " norm_out")
    assert_stats_exact(y.gn_partial, y, c.what + " norm_out")
    if hn is not None:
        y3 = c.ref.reshape(B, 64, Cout)
        _, _, var = fo.group_norm64(y3, gamma, beta, G)
        assert float(var.min()) >= fo.MIN_VAR, c.what
        hn64, _, _ = fo.group_norm64(y3, gamma, beta, G)
        worst = fo.check_elements(hn, hn64, hn64, BF16, f"{c.what} G{G} y_norm")
        print(f"[exact] y_norm {c.what} G{G}: error / tolerance {worst:.3f}")


@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("C,Cout,sc,applied", [(384, 384, None, True), (768, 384, None, False), (384, 384, (384, 384), True)])
def test_norm_out_leaves_output_and_statistics_exact(B, C, Cout, sc, applied):
    """norm_out set (8^2 planes, bf16: the epilogue also applies the GroupNorm that follows): the plain output y and its statistics
    are still exact, and where `norm_applied` is attached it is held element by element to the float64 GroupNorm of that exact y
    (per-channel gamma / beta; tests/fusednorm_oracle.py: 2^-8 |ref| + 2^-16 max|hn|).  applied: at batch 64 the one-sample tile with
    the whole K per workgroup normalises in its epilogue (768 -> 384 splits K there: the wrapper then attaches nothing).  With a
    shortcut the call is the three-tap fold at both batches (afldm_conv2d_shortcut_ok == 2).  These cases keep the weight density of
    the exact file (sigma of a group ~ 30, outside the oracle's sigma <= 12 window, which is a matter of sensitivity, not of the
    tolerance's validity); the cases inside the window are those of tests/test_gpu_fused_norm_exact.py."""
    _norm_out(B, C, Cout, 32, sc, B == 64 and applied)


# afldm_conv2d_norm_ok among Cin = Cout in {96, 192, 384, 768} and G in {8, 32} (bf16, 8^2): 192 from batch 54, 384 from batch 41,
# 768 from batch 21 but not at 64 (another tile takes it there), 96 never, whatever G is (fusednorm_oracle.NORM_OK_FROM; the host file
# asserts this list).  Each accepted pair at the first batch that reports 1 and, where 64 does too, at 64.
NORM_OUT_MORE = [(54, 192, 8), (64, 192, 8), (54, 192, 32), (64, 192, 32), (41, 384, 8), (64, 384, 8), (41, 384, 32),
                 (21, 768, 8), (21, 768, 32)]


@pytest.mark.parametrize("B,C,G", NORM_OUT_MORE)
def test_norm_out_other_groups_and_first_batches(B, C, G):
    """The other (Cout, G) afldm_conv2d_norm_ok accepts (NORM_OUT_MORE), at the smallest batch at which it reports 1 beside 64:
    6 / 12 / 24 / 48 / 96 channels per group."""
    assert B in (fo.NORM_OK_FROM[C], 64)
    _norm_out(B, C, C, G, None, True)


def _resample_exact(c, dtype, want_stats=True):
    ops = _ops()
    o = operands(c, dtype)
    if c.form == "s2":
        y = ops.conv2d_s2(o["x1"], o["w"], o["bias"], pad=c.pad, want_stats=want_stats)
    else:
        w_up2 = ops.pack_weight_up2(c.w.permute(0, 3, 1, 2).contiguous().cuda(), dtype)
        assert float(w_up2.float().abs().max()) <= 4
        y = ops.conv2d_up2(o["x1"], w_up2, o["bias"], want_stats=want_stats)
    assert_exact(y, c.ref, f"{c.what} pad {c.pad} {dtype}")
    if want_stats:
        assert_stats_exact(y.gn_partial, y, f"{c.what} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", xo.RESAMPLE_EXACT, ids=lambda r: "-".join(str(v) for v in r))
def test_resamplers_exact(dtype, r):
    """conv2d_s2 with pads (1, 1) and (0, 1), conv2d_up2 through pack_weight_up2 (its folded taps are sums of at most four ternary
    weights: integers in [-4, 4], exact in bf16), even and odd plane sides."""
    _resample_exact(xo.resample_case(*r), dtype)


# ================================================================================================ f. tail shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(xo.TAIL_EXACT))
def test_tail_shapes_exact(dtype, name):
    """The smallest shapes at which each family can go wrong: 3 x 5 x 7 with 96 couts, the direct conv_in kernel (4 -> 64 at 12^2),
    the MFMA conv_in (4 -> 192 at 32^2, bf16), conv_out (192 -> 4), couts that are no multiple of the N tile.  The kernel family is
    asserted: afldm_conv2d_variant gives -2 for the small-Cin kernels, -16 for skinny.hip (the 192-row 1x1 case), a tile id for the
    GEMM path (conv_out at this size is a split-K GEMM, not the small-Cout kernel);
    k_conv_cin4_mfma writes one statistics record per 128 pixels (8 at 32^2) where the direct kernel leaves them to the stand-alone
    pass (32 at 32^2, 4 at 12^2)."""
    c = conv_case(**xo.TAIL_EXACT[name])
    y, o = run_exact(c, dtype, what=name)
    code = variant_code(c, o, y)
    if name.startswith("conv_in"):
        assert code == -2, code
        S = {"conv_in_direct": 4, "conv_in_mfma": 8 if dtype == BF16 else 32}[name]
        assert y.gn_partial.shape[1] == S, (name, dtype, tuple(y.gn_partial.shape))
    elif name == "ragged_n_tile_1x1":
        assert code == -16, code
    else:
        assert code >= 0, code


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C1,C2,Cout,res,temb", [
    (1, 1, 1, 768, 0, 1408, False, False),       # M = 1 linear (the batched time_emb_proj)
    (64, 1, 1, 192, 0, 768, False, False),       # M = 64 linear (the time MLP)
    (16, 1, 1, 3072, 0, 3072, True, True),       # a 2^2-level convolution in its dense form
    (8, 2, 2, 768, 768, 768, True, False),       # two inputs, 8 samples of 4 pixels in one 64-row block
    (5, 4, 4, 256, 0, 96, True, True),           # 80 rows: a ragged second block
    (40, 2, 2, 768, 0, 768, True, False),        # to_out at the 2^2 level: 16 samples per 64-row block, ragged last block
    (24, 4, 4, 768, 0, 768, True, False),        # to_out at the 4^2 level, 384 rows: the 64 x 64 GEMM tile with 4 whole samples each
])
def test_few_rows_linear_exact(dtype, B, H, W, C1, C2, Cout, res, temb):
    """1x1 convolutions / dense layers over few rows: taken by skinny.hip (afldm_conv2d_variant == -16), the last case by the
    64 x 64 GEMM tile (variant 32) that holds several whole samples."""
    c = conv_case(B, H, W, C1, C2, Cout, 1, temb=temb, residual=res)
    y, o = run_exact(c, dtype, what="few rows")
    code = variant_code(c, o, y)
    if B * H * W == 384:
        assert code >= 0 and code & 255 == 32, f"{c.what} {dtype}: variant 32 did not take the call (code {code})"
    else:
        assert code == -16, f"{c.what} {dtype}: skinny.hip did not take the call (code {code})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C1,C2,Cout,B", [(64, 0, 64, 5), (96, 32, 48, 5), (768, 0, 768, 40)])
def test_2x2_plane_as_dense_layer_exact(dtype, C1, C2, Cout, B):
    """blocks.conv_forward on a 2^2 plane: the dense re-formulation (its weights are sums of the taps that fall on one input pixel -
    here one tap each, so still ternary) with virtual concat, the per-channel time embedding (temb_mod), residual, statistics."""
    import torch.nn as nn
    from afldm_amd.models import blocks
    c = conv_case(B, 2, 2, C1, C2, Cout, 3, temb=True, residual=True)
    o = operands(c, dtype)
    conv = nn.Conv2d(C1 + C2, Cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(c.w.permute(0, 3, 1, 2))
        conv.bias.copy_(c.bias)
    conv = conv.cuda()
    xin = o["x1"] if C2 == 0 else (o["x1"], o["x2"])
    y = blocks.conv_forward(conv, xin, temb=o["temb"], temb_stride=Cout, residual=o["residual"], want_stats=True)
    assert ("dense2x2", dtype, C1, C2) in conv.__dict__["_afldm_cache"]
    # the dense form is one linear layer over B rows: skinny.hip runs it at B = 5, the 64 x 64 GEMM tile (variant 32) at B = 40, K = 3072
    w2, b2 = blocks.packed_conv_dense2x2(conv, dtype, C1, C2)
    probe = _ops().conv_args(o["x1"].reshape(B, 4 * C1), w2, b2, None if C2 == 0 else o["x2"].reshape(B, 4 * C2), o["temb"], Cout,
                             o["residual"].reshape(B, 4 * Cout), y.view(B, 4 * Cout), temb_mod=Cout)
    code = _lib().lib.afldm_conv2d_variant(ctypes.byref(probe))
    if B == 40:
        assert code >= 0 and code & 255 == 32, f"the dense form of {c.what} {dtype} did not run on variant 32 (code {code})"
    else:
        assert code == -16, f"the dense form of {c.what} {dtype} did not run on skinny.hip (code {code})"
    assert_exact(y, c.ref, c.what + " dense 2x2")
    assert_stats_exact(y.gn_partial, y, c.what + " dense 2x2")


# ================================================================================================ g. the fused UNet tail
@pytest.mark.parametrize("C", [64, 128, 192])
def test_conv_out_fused_exact(C):
    """afldm_conv_out_fused (GroupNorm-apply -> SiLU -> 3 x 3 convolution to <= 4 couts in one launch) bit for bit against the
    float64 reference of addressed_oracle.tail_case: Cout 1 .. 4, G in {16, 32, 64}, B = 3, the fabricated partials in 1, 3 and 9
    ragged splits (gn_channel_sums: its tail loop alone, and 8 + 1).  A kernel that activated its zero padding is off by at
    least 8 on every border pixel; one that took another sample's or group's statistics is off on whole planes."""
    ops = _ops()
    fails = Failures()
    for Cout, G in ado.tail_grid(C):
        c = ado.tail_case(ado.TAIL_B, C, Cout, G)
        x, w, bias = dev(c.x, BF16), dev(c.w, BF16), dev(c.bias, FP32)
        gamma, beta = dev(c.gamma, FP32), dev(c.beta, FP32)
        for S in ado.SPLITS:
            x.gn_partial = ado.partials(c.m, C, c.N * c.N, S, c.seed).cuda()           # the op takes them from the tensor
            y = ops.conv_out_fused(x, w, bias, gamma, beta, G, ado.EPS)
            assert y is not None and y.shape == (c.B, c.N, c.N, Cout), "conv_out_fused refused the shape"
            fails.run(f"{c.what} S={S}", lambda y=y, c=c, S=S: assert_exact(y, c.ref, f"{c.what} S={S}"))
    fails.check()
