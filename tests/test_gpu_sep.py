"""The large-plane kernels of csrc/sep.hip (and afldm_gn_fold) on MI355X against the float64 oracle of tests/sep_oracle.py,
PER GROUP of 16 lines, at the project's tolerances for them (sep_oracle.TOL).

Every instantiation sep_dispatch can select, against its dispatch table (K, R, R2 | waves | lines per wave):

  fp32  plain CT = 1   (16,32) (32,64) (64,128) (32,16) (64,32) (128,64)                      test_every_dispatched_configuration
        chained full   (16,32,16) (32,64,32) (64,128,64)                                      test_every_dispatched_configuration
        identity, 4 w  (32,64,32) (64,128,64)          [up_identity = 2]                      test_every_dispatched_configuration
  bf16  plain CT = 1   (16,32) (32,64) (64,128) (32,16) (64,32) (128,64) (128,256) (256,128)  ... inner_count 16 / 48 / 112
        plain CT = 4   (32,64) (64,128) (128,256) (64,32)   [inner_count % 64 == 0]           ... inner_count 64 / 448
        plain CT = 2   (128,64) (256,128)                   [inner_count % 32 == 0]           ... inner_count 32 / 224
        chained full   (16,32,16) (32,64,32) (64,128,64) (128,256,128)                        test_every_dispatched_configuration
        identity, 4 w  (32,64,32) (64,128,64)          [up_identity = 2]                      test_every_dispatched_configuration
        identity, 8 w  (128,256,128)                   [up_identity = 1]                      test_every_dispatched_configuration

32 instantiations.  test_more_than_one_sweep runs one launch of 4099 groups per shape class (CT = 1 fp32 / bf16, CT = 2, CT = 4,
chained full, identity 4-wave, identity 8-wave) and wants it bit-identical to the same lines in single-iteration launches; the
GroupNorm table repeats that at 4099 groups (W form) and at 3 x 1367 = 4101 groups (H form, where 4099, a prime, has no shape).

The wide-tile (CT) cases need the library's default dispatch: with AFLDM_SEP_NO_CT set every one of them would run the CT = 1
kernel, so the tests that mean a CT kernel refuse to run under it (_wide_tiles_on)."""
import os

import pytest
import torch
import torch.nn.functional as F

import sep_oracle as so

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
NAME = {F32: "fp32", BF16: "bf16"}
_MATS = {}


def _ops():
    from afldm_amd import ops
    return ops


def _mats(K, R, R2=0):
    """(M, M2) host, (M, M2) device"""
    if (K, R, R2) not in _MATS:
        M, M2 = so.matrices(K, R, R2)
        _MATS[K, R, R2] = (M, M2, M.cuda(), None if M2 is None else M2.cuda())
    return _MATS[K, R, R2]


def _dev(x, dtype):
    return x.to(device="cuda", dtype=dtype)


def _run(x, K, R, R2=0, y=None, table=None, C=0, outer_per_sample=1, act=0, up_identity=0):
    """afldm_sep_pass on x [outer, K, inner] (device; any view whose last dimension is contiguous) -> y [outer, R2 or R, inner].
    A fresh y is NaN-filled: a group that is never written fails the finiteness check of group_errors."""
    outer, Kx, inner = x.shape
    assert Kx == K and x.stride(2) == 1
    _, _, Md, M2d = _mats(K, R, R2)
    if y is None:
        y = torch.full((outer, R2 or R, inner), float("nan"), dtype=x.dtype, device="cuda")
    assert tuple(y.shape) == (outer, R2 or R, inner) and y.stride(2) == 1
    _ops().sep_pass(x, y, Md, K, R, outer, inner, x.stride(0), x.stride(1), y.stride(0), y.stride(1), M2=M2d, R2=R2,
                    gn_table=table, C=C, outer_per_sample=outer_per_sample, act=act, up_identity=up_identity)
    return y


def _ref(x, K, R, R2=0, **kw):
    M, M2, _, _ = _mats(K, R, R2)
    return so.sep_reference(x, M, M2, **kw)


def _check(what, got, ref, bound, lines=16):
    _, worst = so.group_errors(got.float().cpu(), ref, lines)
    print(f"[sep] {what}: worst group rel-RMS {worst:.2e} (bound {bound:.1e})")
    assert worst <= bound, (what, worst, bound)
    return worst


def _wide_tiles_on():
    assert "AFLDM_SEP_NO_CT" not in os.environ, "AFLDM_SEP_NO_CT switches the wide-tile kernels off: these cases would not run them"


def _identities(K, R2):
    if not R2:
        return [0]
    return [0] + ([2] if K in (32, 64) else []) + ([1] if K == 128 else [])


# ------------------------------------------------------------------------------------------------ a. every configuration
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("K,R,R2", so.configs(BF16), ids=lambda v: str(v))
def test_every_dispatched_configuration(K, R, R2, dtype):
    """Small launches (21 or 61 groups: the last workgroup starts with idle waves) in two layouts: W form, one group per outer
    (in_k_stride = inner_count = lines per wave); H form, 7 groups per outer, output strides != input strides (R != K).  bf16
    plain passes with a wide-tile kernel run with an inner_count that selects it and with 16 / 48 / 112, which do not; plain
    passes also with act = 1; chained passes also in the identity form where the size has one."""
    if (K, R, R2) not in so.configs(dtype):
        with pytest.raises(RuntimeError, match="no kernel for"):         # fp32: the 128 / 256 matrices do not fit the LDS
            _run(_dev(so.lines(1, K, 16, dtype), dtype), K, R, R2)
        return
    _wide_tiles_on()
    ct = so.CT.get((K, R)) if dtype == BF16 and not R2 else None
    shapes = [("W", 61, 16), ("H", 3, 7 * 16)]
    if ct:
        shapes += [(f"W/CT{ct}", 61, 16 * ct), (f"H/CT{ct}", 3, 7 * 16 * ct), ("W/48", 7, 48)]
    bound = so.tol(dtype, R2)
    for label, outer, inner in shapes:
        x = so.lines(outer, K, inner, dtype, seed=K + R + inner)
        xd = _dev(x, dtype)
        for act in ((0,) if R2 else (0, 1)):
            ref = _ref(x, K, R, R2, act=act)
            for ident in _identities(K, R2):
                y = _run(xd, K, R, R2, act=act, up_identity=ident)
                _check(f"{NAME[dtype]} K={K} R={R} R2={R2} {label} {outer}x{inner} act={act} identity={ident}", y, ref, bound)


# ------------------------------------------------------------------------------------------------ b. more than one sweep
SWEEPS = [("CT1-fp32", F32, 32, 64, 0, 16, 0), ("CT1-bf16", BF16, 32, 64, 0, 16, 0), ("CT2", BF16, 128, 64, 0, 32, 0),
          ("CT4", BF16, 128, 256, 0, 64, 0), ("CT4-act", BF16, 64, 32, 0, 64, 0), ("chained-fp32", F32, 16, 32, 16, 16, 0),
          ("chained-bf16", BF16, 64, 128, 64, 16, 0), ("identity-4wave-fp32", F32, 32, 64, 32, 16, 2),
          ("identity-4wave-bf16", BF16, 64, 128, 64, 16, 2), ("identity-8wave", BF16, 128, 256, 128, 16, 1)]


@pytest.mark.parametrize("label,dtype,K,R,R2,inner,ident", SWEEPS, ids=[s[0] for s in SWEEPS])
def test_more_than_one_sweep(label, dtype, K, R, R2, inner, ident):
    """One launch of 4099 groups (one per outer): every wave runs at least three iterations of the pipelined loop - the
    prefetch of the next group under the current one, the reuse of the prefetch registers - and the last iteration has three
    live waves in workgroup 0.  Bit for bit the same lines in launches of at most 512 groups (one iteration each, same
    kernel, same per-group arithmetic); the first 512 groups, the last 16 and 16 either side of every sweep boundary
    against float64."""
    _wide_tiles_on()
    n = so.SWEEP_GROUPS
    act = 1 if label.endswith("act") else 0
    x = so.lines(n, K, inner, dtype, seed=n + K)
    xd = _dev(x, dtype)
    kw = dict(act=act, up_identity=ident)
    y = _run(xd, K, R, R2, **kw)
    y2 = torch.full_like(y, float("nan"))
    for o in range(0, n, 512):
        _run(xd[o:o + 512], K, R, R2, y=y2[o:o + 512], **kw)
    same = torch.equal(y, y2)
    if not same:
        bad = (y != y2).flatten(1).any(1).nonzero().flatten().tolist()
        print(f"[sep] {label}: {len(bad)} groups differ from their single-iteration launch, first {bad[:8]} last {bad[-8:]}")
    assert same
    idx = torch.tensor(so.sweep_checkpoints(n))
    _check(f"{label} 4099 groups, {len(idx)} of them vs fp64", y[idx.cuda()], _ref(x[idx], K, R, R2, act=act),
           so.tol(dtype, R2))


# ------------------------------------------------------------------------------------------------ c. CT kernel == its CT = 1 sibling
@pytest.mark.parametrize("K,R", sorted(so.CT), ids=lambda v: str(v))
def test_wide_tile_kernel_equals_its_16_line_sibling_bit_for_bit(K, R):
    """[outer, K, 16 CT] through the CT kernel once, and as CT launches on the column slices x[..., 16q : 16q + 16]
    (inner_count = 16: the CT = 1 kernel; same strides, 32-byte pointer offsets) into the matching slices of y.  Both
    accumulate over k in the same order."""
    _wide_tiles_on()
    ct = so.CT[K, R]
    x = so.lines(13, K, 16 * ct, BF16, seed=K)
    xd = _dev(x, BF16)
    for act in (0, 1):
        y = _run(xd, K, R, act=act)
        ys = torch.full_like(y, float("nan"))
        for q in range(ct):
            _run(xd[..., 16 * q:16 * q + 16], K, R, y=ys[..., 16 * q:16 * q + 16], act=act)
        assert torch.equal(y, ys), (K, R, act)
        _check(f"CT{ct} K={K} R={R} act={act}", y, _ref(x, K, R, act=act), so.TOL["plain"])


# ------------------------------------------------------------------------------------------------ d. fused GroupNorm table
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("C", [8, 16, 48, 80])
def test_fused_groupnorm_table(C, dtype):
    """B = 3 samples with distinct tables.  H form: inner_count = N C, a sample per outer (bf16: the CT = 4 kernel, whose
    64-line groups straddle pixels unless 64 % C == 0; fp32: CT = 1).  W form: inner_count = C rounded up to 16 (C = 8: two
    periods per group), N outers per sample."""
    _wide_tiles_on()
    B, N = 3, 32
    tab = so.gn_tables(B, C, seed=C)
    tabd = tab.cuda()
    bound = so.tol(dtype)
    for label, outer, inner, per in (("H", B, N * C, 1), ("W", B * N, -(-C // 16) * 16, N)):
        x = so.lines(outer, N, inner, dtype, seed=C + inner)
        y = _run(_dev(x, dtype), N, 2 * N, table=tabd, C=C, outer_per_sample=per)
        ref = _ref(x, N, 2 * N, table=tab, C=C, outer_per_sample=per)
        _check(f"{NAME[dtype]} table C={C} {label} {outer}x{inner}", y, ref, bound)


@pytest.mark.parametrize("K,R,N", [(64, 128, 64), (128, 64, 2), (16, 32, 16), (64, 32, 64)], ids=lambda v: str(v))
def test_fused_groupnorm_table_bf16_groups_that_straddle_pixels(K, R, N):
    """C = 48, bf16: the CT = 4 kernels at K = 64 (64-line groups over pixels of 48 channels), the CT = 2 kernel with
    inner_count = 96, the CT = 1 kernel at K = 16"""
    _wide_tiles_on()
    B, C = 3, 48
    tab = so.gn_tables(B, C, seed=K)
    x = so.lines(B, K, N * C, BF16, seed=K + 7)
    y = _run(_dev(x, BF16), K, R, table=tab.cuda(), C=C)
    _check(f"bf16 table C=48 K={K} R={R} inner={N * C}", y, _ref(x, K, R, table=tab, C=C), so.TOL["plain"])


def test_fused_groupnorm_table_more_than_one_sweep_w_form():
    """4099 groups (fp32, one per outer, 1367 outers per sample, C = 16) against launches that stay inside one sample and
    one sweep: the table entries of the NEXT group are prefetched with its lines."""
    n, K, R, C, per = so.SWEEP_GROUPS, 32, 64, 16, 1367
    tab = so.gn_tables(3, C, seed=1)
    tabd = tab.cuda()
    x = so.lines(n, K, 16, F32, seed=99)
    xd = _dev(x, F32)
    y = _run(xd, K, R, table=tabd, C=C, outer_per_sample=per)
    y2 = torch.full_like(y, float("nan"))
    for b in range(3):
        for o in range(b * per, min((b + 1) * per, n), 512):
            o1 = min(o + 512, (b + 1) * per, n)
            _run(xd[o:o1], K, R, y=y2[o:o1], table=tabd[b:b + 1], C=C, outer_per_sample=per)
    assert torch.equal(y, y2)
    _check("fp32 table W form 4099 groups", y, _ref(x, K, R, table=tab, C=C, outer_per_sample=per), so.TOL["fp32"])


def test_fused_groupnorm_table_more_than_one_sweep_h_form():
    """3 samples of 1367 groups (bf16, C = 48: the channel of a lane changes from group to group with period 3) against
    launches on 165-group column slices (3 x 165 groups a launch: one iteration), which start on a pixel and, like the whole,
    are no multiple of 64 lines wide: the same CT = 1 kernel"""
    B, K, R, C, groups = 3, 32, 64, 48, 1367
    tab = so.gn_tables(B, C, seed=2)
    tabd = tab.cuda()
    x = so.lines(B, K, groups * 16, BF16, seed=98)
    xd = _dev(x, BF16)
    y = _run(xd, K, R, table=tabd, C=C)
    y2 = torch.full_like(y, float("nan"))
    for i in range(0, groups * 16, 165 * 16):
        i1 = min(i + 165 * 16, groups * 16)
        assert i % C == 0 and (i1 - i) % 64 != 0
        _run(xd[..., i:i1], K, R, y=y2[..., i:i1], table=tabd, C=C)
    assert torch.equal(y, y2)
    _check("bf16 table H form 4101 groups", y, _ref(x, K, R, table=tab, C=C), so.TOL["plain"])


# ------------------------------------------------------------------------------------------------ e. afldm_gn_table
@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (50.0, 1.0)], ids=["mean0", "mean50"])
@pytest.mark.parametrize("C,G,S,B", [(32, 8, 4, 2), (64, 4, 4, 2), (96, 8, 7, 3), (96, 3, 1, 3), (512, 4, 1, 2), (512, 4, 32, 2),
                                     (128, 32, 512, 1)], ids=lambda v: str(v))
def test_gn_table_vs_fp64_on_the_same_partials(C, G, S, B, mean, std):
    """cpg S = 16 / 64 / 84 partials over 64 lanes, 9 waves in 3 workgroups, cpg = 128 (two table entries per lane), S = 512.
    mean 50 / std 1: E[x^2] - m^2 loses 3.4 digits, harmless only because the kernel combines the partials in fp64."""
    st, HW = so.partials(B, S, C, 4, mean=mean, std=std, seed=C + S)
    gamma, beta = so.affine(C, seed=S)
    eps = 1e-6
    got = _ops().gn_table(_ops().GNStats(st.cuda()), gamma.cuda(), beta.cuda(), B, C, G, HW, eps).double().cpu()
    ref = so.gn_table_reference(st, gamma, beta, G, HW, eps)
    assert got.shape == ref.shape == (B, C, 2) and torch.isfinite(got).all()
    es = ((got[..., 0] - ref[..., 0]).abs() / ref[..., 0].abs()).max()
    mean_scale = (beta.double()[None] - ref[..., 1]).abs()                  # |mean * scale|
    et = ((got[..., 1] - ref[..., 1]).abs() / (beta.double().abs()[None] + mean_scale)).max()
    print(f"[gn_table] C={C} G={G} S={S} B={B} mean={mean}: scale {float(es):.2e} shift {float(et):.2e} (bound 1e-5)")
    assert es <= 1e-5 and et <= 1e-5


# ------------------------------------------------------------------------------------------------ f. afldm_gn_fold
def _fold(st, S_out):
    from afldm_amd import _lib
    B, S_in, C, _ = st.shape
    out = torch.full((B, S_out, C, 2), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib.afldm_gn_fold(st.data_ptr(), S_in, out.data_ptr(), S_out, B, C, _lib.stream_ptr()), "gn_fold")
    return out


@pytest.mark.parametrize("S_in,S_out", [(512, 32), (64, 32), (32, 32)])
def test_gn_fold_vs_fp64_sum(S_in, S_out):
    B, C = 2, 20
    st, _ = so.partials(B, S_in, C, 8, mean=1.0, std=2.0, seed=S_in)
    got = _fold(st.cuda(), S_out).double().cpu()
    r = S_in // S_out
    bound = r * 2.0 ** -24 * st.double().abs().view(B, S_out, r, C, 2).sum(2)          # an fp32 sum of r terms
    err = (got - so.fold_reference(st, S_out)).abs()
    print(f"[gn_fold] {S_in}->{S_out}: worst error / bound {float((err / bound).max()):.2f}")
    assert torch.isfinite(got).all() and (err <= bound).all()
    if r == 1:
        assert torch.equal(got.float(), st)


def test_gn_fold_refuses_a_ragged_split():
    st, _ = so.partials(2, 48, 20, 2)
    with pytest.raises(RuntimeError, match="S_in=48 must be a multiple of S_out=32"):
        _fold(st.cuda(), 32)
    assert torch.equal(_fold(st.cuda(), 48).cpu(), st)


# ------------------------------------------------------------------------------------------------ g. afldm_softmax_rows
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("cols", [1, 8, 255, 256, 257, 1000, 1024, 4099])
def test_softmax_rows(cols, dtype):
    """Column counts around the 256-thread stride, scales 1 / 512^-0.5 / -1; rows: randn * 4, a logit 60 nats above the rest at
    index 0 and at cols - 1 (argmax exact), a constant row, and in fp32 a row offset by +3e4.  Per row, at the tolerances of
    test_attention (test_gpu_ops.close)."""
    from test_gpu_ops import close
    for scale in (1.0, 512 ** -0.5, -1.0):
        x, names = so.softmax_rows(cols, scale, dtype)
        y = _ops().softmax_rows(_dev(x, dtype), scale).float().cpu()
        ref = so.softmax_reference(x, scale)
        assert y.shape == ref.shape == (5, cols)
        for r, name in enumerate(names):
            err = float((y[r].double() - ref[r]).abs().max() / ref[r].abs().max())
            print(f"[softmax] {NAME[dtype]} cols={cols} scale={scale:.4f} {name}: max/scale {err:.2e}")
            close(y[r], ref[r], dtype, f"softmax cols={cols} scale={scale} {name}", f32_tol=5e-5, bf16_rms=1e-2)
            if name.startswith("spike@"):
                assert int(y[r].argmax()) == int(name[6:]) and float(y[r].max()) == 1.0
        assert (y.double().sum(-1) - 1).abs().max() <= (1e-5 if dtype == F32 else 1e-2)


# ------------------------------------------------------------------------------------------------ h. composed paths
def _nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(device="cuda", dtype=dtype)


def _as_lines(t):
    """NCHW (cpu) or NHWC (device) planes -> [B H, W, C] float64 on the CPU"""
    if t.is_cuda:
        return so.planes_as_lines(t.float().cpu())
    return so.planes_as_lines(t.permute(0, 2, 3, 1))


@pytest.mark.parametrize("N,B,C,G,dtype", [(64, 3, 48, 8, F32), (64, 3, 48, 8, BF16), (128, 2, 64, 4, BF16)],
                         ids=lambda v: NAME.get(v, str(v)))
def test_large_plane_activation_with_statistics(N, B, C, G, dtype):
    """ops.af_act (GroupNorm table + up-H, chained W, down-H) at three samples of 48 channels (groups of the H passes straddle
    pixels, CT off in the W pass) and at 64 channels on 128^2 planes, per 16 channels of a pixel row"""
    from oracle import ideal_filters as idf
    ops = _ops()
    x = so.planes(B, C, N, dtype, seed=N + C)
    gamma, beta = so.affine(C, seed=N)
    ref = idf.warped_nonlinearity(F.group_norm(x.double(), G, gamma.double(), beta.double(), 1e-6))
    xh = _nhwc(x, dtype)
    y = ops.af_act(xh, None, ops.gn_stats(xh, G), gamma.cuda(), beta.cuda(), G, 1e-6)
    _check(f"{NAME[dtype]} af_act N={N} B={B} C={C} G={G}", _as_lines(y), _as_lines(ref), so.tol(dtype, composed=True))


def test_large_plane_activation_takes_folded_512_split_statistics():
    """Statistics as a convolution on a 256^2 plane leaves them - 512 partials per sample, folded to 32 - give the activation
    that ops.gn_stats gives, within the fp32 tolerance"""
    ops = _ops()
    N, B, C, G = 64, 2, 32, 8
    x = so.planes(B, C, N, F32, seed=5)
    gamma, beta = so.affine(C, seed=6)
    xh = _nhwc(x, F32)
    xs = x.double().permute(0, 2, 3, 1).reshape(B, 512, N * N // 512, C)
    st512 = torch.stack([xs.sum(2), xs.pow(2).sum(2)], -1).float().cuda()
    folded = _fold(st512, 32)
    y_fold = ops.af_act(xh, None, ops.GNStats(folded), gamma.cuda(), beta.cuda(), G, 1e-6)
    y = ops.af_act(xh, None, ops.gn_stats(xh, G), gamma.cuda(), beta.cuda(), G, 1e-6)
    _check("af_act with folded statistics vs gn_stats", _as_lines(y_fold), _as_lines(y).double(), so.TOL["fp32"])


@pytest.mark.parametrize("B,C", [(3, 48), (2, 64)], ids=lambda v: str(v))
@pytest.mark.parametrize("dtype,N", [(F32, 32), (F32, 64), (BF16, 32), (BF16, 64), (BF16, 128)],
                         ids=lambda v: NAME.get(v, str(v)))
def test_large_plane_resample_batched(dtype, N, B, C):
    """ops.af_up2 / ops.af_lpf_down2: C = 48 keeps the W pass on 16-line groups, C = 64 puts it on the wide tiles"""
    from oracle import ideal_filters as idf
    ops = _ops()
    x = so.planes(B, C, N, dtype, seed=N + B)
    xh = _nhwc(x, dtype)
    bound = so.tol(dtype)
    _check(f"{NAME[dtype]} af_up2 N={N} B={B} C={C}", _as_lines(ops.af_up2(xh)), _as_lines(idf.upsample_rfft(x.double(), 2)), bound)
    _check(f"{NAME[dtype]} af_lpf_down2 N={N} B={B} C={C}", _as_lines(ops.af_lpf_down2(xh)),
           _as_lines(idf.lpf_rfft(x.double())[:, :, ::2, ::2]), bound)


# ------------------------------------------------------------------------------------------------ i. errors
def test_bad_arguments_are_reported_and_the_library_stays_usable():
    """Argument checks that return before any launch; a valid call afterwards still matches the oracle."""
    ops = _ops()
    K, R = 32, 64
    x = so.lines(5, K, 32, F32, seed=3)
    xd = _dev(x, F32)
    M, M2, Md, M2d = _mats(K, R, 32)
    tab = so.gn_tables(1, 16).cuda()
    y = torch.zeros(5, R, 32, device="cuda")
    big = torch.zeros(5 * R * 32 + 8, device="cuda")
    plain = lambda **kw: ops.sep_pass(**{**dict(x=xd, y=y, M=Md, K=K, R=R, outer_count=5, inner_count=32, in_outer_stride=K * 32,
                                                in_k_stride=32, out_outer_stride=R * 32, out_k_stride=32), **kw})
    with pytest.raises(RuntimeError, match="no kernel for K=128 R=256 R2=0 in this dtype"):
        x128 = torch.zeros(1, 128, 16, device="cuda")
        ops.sep_pass(x128, torch.zeros(1, 256, 16, device="cuda"), _mats(128, 256)[2], 128, 256, 1, 16, 128 * 16, 16, 256 * 16, 16)
    with pytest.raises(RuntimeError, match="inner_count=24 must be a positive multiple of 16"):
        plain(inner_count=24)
    with pytest.raises(RuntimeError, match="input strides must keep 16-byte chunks aligned"):
        plain(in_k_stride=4)
    with pytest.raises(RuntimeError, match="output strides must keep 16-byte chunks aligned"):
        plain(y=big[2:2 + 5 * R * 32].view(5, R, 32))                      # 8 bytes past a 16-byte boundary
    with pytest.raises(RuntimeError, match="GN table needs C and outer_per_sample"):
        plain(gn_table=tab, C=0)
    with pytest.raises(RuntimeError, match="R2 > 0 needs M2"):
        plain(R2=32)
    assert float(y.abs().max()) == 0.0 and float(big.abs().max()) == 0.0   # nothing was launched
    _check("valid call after the refusals", _run(xd, K, R), _ref(x, K, R), so.TOL["fp32"])
