"""Every batch position, bit for bit (MI355X): the relations of tests/batch_oracle.py on the FFHQ alias-free UNet at the
benchmark batch sizes and on every kernel that puts several samples into one workgroup / tile or switches its plan on the batch.

    rotation   f(roll(x, r)) == roll(f(x), r)             torch.equal, every output (GroupNorm partial sums included)
    poison     sample p all NaN (or 1e4 x its data):      every other sample's output unchanged, torch.equal

Inputs come from batch_oracle.distinct_batch: every sample has its own scale and offset, so a neighbour's GroupNorm
statistics, time-embedding row or halo row moves a sample by O(1), and nothing here has a tolerance.  The golden forward of
tests/test_gpu_unet.py, placed at eight positions of a batch of 64, anchors the values; the rotations carry that verdict to
every position.

Kernel level: `g` = samples of one workgroup / tile, read from the kernel's source (the table at each test); batches g + 1 and
2 g + 1 put a sample into the last slot of the first workgroup and the first slot of the second, with a ragged last one; where
the tile only exists for whole multiples of g (the halo-patch tiles: M % BM == 0) 2 g and 3 g run as well, and where a policy
switches on the batch, that batch.  Rotations by 1 and 5; NaN at the first sample, the last, and slots g - 1 and g together.
"""
import ctypes
import math
import time

import pytest
import torch

import batch_oracle as bo
from test_gpu_unet import FWD_TOL, build, rel_rms

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]

# Kernels whose ROUNDING legitimately depends on the slot a sample has inside a workgroup: name -> (g, "file:line: why").  For
# these, check_poison and rotations by multiples of g stay exact; the other rotations compare per sample against a float64
# reference at the bound of the kernel's own value test.  Empty: no kernel of this file needs it.
SLOT_DEPENDENT = {}


def _ops():
    from afldm_amd import ops
    return ops


def _id(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, (tuple, list)):
        return "-".join(_id(i) for i in v)
    return str(v)


def dev(t, dtype=None):
    return t.to(device="cuda", dtype=dtype or t.dtype).contiguous()


def rand_w(shape, fan_in, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return dev(torch.randn(shape, generator=g) / fan_in ** 0.5, dtype)


def rand_v(n, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return dev(torch.randn(n, generator=g) * scale + offset)


def relations(what, f, x, g, rotations=(1, 5)):
    """The kernel-level relations on f at the batch of x: rotations, NaN at the first / last sample and at slots (g - 1, g)."""
    assert what.split()[0] not in SLOT_DEPENDENT, "a slot-dependent kernel needs its float64 reference here"
    xs = x if isinstance(x, tuple) else (x,)
    B = xs[0].shape[0]
    base = bo.run(f, xs)
    for o in base:
        assert torch.isfinite(o).all(), f"{what} B={B}: the clean run is not finite"
    for r in sorted({r % B for r in rotations} - {0}):
        bo.check_rotation(f, xs, r, base=base, what=f"{what} B={B}")
    seam = tuple(sorted({min(g - 1, B - 1), min(g, B - 1)}))
    for p in (0, B - 1, seam):
        bo.check_poison(f, xs, p, math.nan, base=base, what=f"{what} B={B}")
    torch.cuda.synchronize()


# =============================================================================================== model level
_T0 = []


@pytest.fixture(scope="module", autouse=True)
def _clock():
    _T0.append(time.time())
    yield


ROTATIONS = (1, 3, 8, 16, 17, 32)


@pytest.fixture(scope="module")
def ffhq():
    """The FFHQ alias-free UNet, built once per dtype (test_gpu_unet.build)."""
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = build("ffhq", dtype)[0]
        return cache[dtype]
    return get


def _latents(B, seed=1):
    return dev(bo.distinct_batch(B, (4, 32, 32), seed))


def _rotations(B):
    return sorted({r for r in ROTATIONS + (B - 1,) if 0 < r < B})


@pytest.mark.parametrize("dtype,B", [(BF16, 8), (BF16, 16), (BF16, 32), (BF16, 64), (F32, 64)], ids=_id)
def test_unet_rotation(ffhq, dtype, B):
    """Eager forward, one timestep for all samples: every rotation of the batch rotates the output, bit for bit."""
    unet = ffhq(dtype)
    f = lambda x: unet(x, 501, return_dict=False)[0]
    x = _latents(B)
    base = None
    for r in _rotations(B):
        base = bo.check_rotation(f, x, r, base=base, what=f"FFHQ UNet {_id(dtype)} B={B}")
    assert torch.isfinite(base[0]).all()


def test_unet_rotation_with_a_timestep_per_sample(ffhq):
    """bf16, batch 64, a [B] tensor of timesteps rolled along with the latents (the time-embedding rows have a stride)."""
    unet = ffhq(BF16)
    f = lambda x, t: unet(x, t, return_dict=False)[0]
    B = 64
    ts = dev(torch.arange(B, dtype=torch.float32) * 15 + 11)
    x = (_latents(B, seed=2), ts)
    base = None
    for r in _rotations(B):
        base = bo.check_rotation(f, x, r, base=base, what="FFHQ UNet bf16 B=64, timestep per sample")
    assert torch.isfinite(base[0]).all()


@pytest.mark.parametrize("B", [64, 8])
def test_unet_poison(ffhq, B):
    """bf16: one sample all NaN, or 1e4 times its data - every other sample's output is unchanged, bit for bit."""
    unet = ffhq(BF16)
    f = lambda x: unet(x, 501, return_dict=False)[0]
    x = _latents(B, seed=3)
    base = bo.run(f, x)
    assert torch.isfinite(base[0]).all()
    for p in (0, 7, 8, 15, 16, 37, 63):
        if p < B:
            bo.check_poison(f, x, p, math.nan, base=base, what=f"FFHQ UNet bf16 B={B}")
    for p in (0, 16, 63):
        if p < B:
            bo.check_poison(f, x, p, bo.BIG, base=base, what=f"FFHQ UNet bf16 B={B}")


ANCHORS = (0, 1, 15, 16, 37, 38, 62, 63)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_unet_anchor_positions_against_the_oracle(ffhq, golden, dtype):
    """The sample of the oracle's fixture (g6_ffhq_unet.npz, t = 981) at eight positions of a batch of 64 whose other samples
    are distinct_batch: each position within FWD_TOL of the oracle's output (metric and bound of
    test_ffhq_unet_forward_and_cross_frame_load)."""
    g = golden("g6_ffhq_unet.npz")
    gx, gy = torch.from_numpy(g["x"]), g["y_t981"]
    x = bo.distinct_batch(64, (4, 32, 32), 4)
    src = {p: i % gx.shape[0] for i, p in enumerate(ANCHORS)}
    for p, i in src.items():
        x[p] = gx[i]
    y = ffhq(dtype)(dev(x), 981, return_dict=False)[0]
    assert torch.isfinite(y).all()
    for p, i in src.items():
        r = rel_rms(y[p:p + 1], gy[i:i + 1])
        print(f"[anchor {_id(dtype)}] position {p}: rel-RMS {r:.3e} (bound {FWD_TOL[dtype]})")
        assert r <= FWD_TOL[dtype], (p, r)


def test_replayed_graph_rotation(ffhq):
    """Three DDIM steps of the graph-replayed engine at batch 64 (bf16) from x and from roll(x, 17): the latents roll."""
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet = ffhq(BF16)
    x = bo.distinct_batch(64, (4, 32, 32), 5)
    eng = DenoiseEngine(unet, ffhq_ddim_scheduler(), 64, 50, use_graph=True)
    outs = []
    for lat in (x, torch.roll(x, 17, 0)):
        eng.reset(lat)
        eng.step(3)
        outs.append(eng.lat.clone())
    assert torch.isfinite(outs[0]).all()
    # (both runs are done: the helper only compares outs[1] with roll(outs[0], 17) and names the positions that differ)
    bo.check_rotation(lambda _: outs[1], x, 17, base=[outs[0]], what="DenoiseEngine graph, 3 steps, B=64")


# =============================================================================================== kernel level
# ----------------------------------------------------------------------------------------------- dense2.hip
# afldm_conv2x2_const_norm_act: D2_ROWS = 16 samples per workgroup (dense2.hip:37, rt = ceil(B / 16) at :239)  ->  g = 16.
# B = 17, 33 (g + 1, 2 g + 1) and 64 (ops._DENSE2_MIN_B, where the policy switches to it).
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("per_sample_temb", [True, False], ids=["temb_rows", "temb_broadcast"])
@pytest.mark.parametrize("B", [17, 33, 64])
def test_conv2x2_const_norm_act(dtype, per_sample_temb, B):
    from afldm_amd.models import blocks
    ops = _ops()
    Cin, Cout, G = 256, 96, 8                 # the smallest case of test_conv2x2_const_norm_act_vs_separate_launches
    assert ops.conv2x2_const_norm_act_ok(Cin, Cout, G, dtype, batch=64)
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=torch.Generator().manual_seed(1)) * (2.0 / (9 * Cin)) ** 0.5)
    conv = conv.cuda()
    w, bias = blocks.packed_conv_dense2x2_const_cm(conv, dtype), blocks._bias_f32(conv)
    gamma, beta = rand_v(Cout, 2, 0.2, 1.0), rand_v(Cout, 3, 0.3)
    a = dev(bo.distinct_batch(B, (Cin,), 10), dtype)
    if per_sample_temb:
        temb = dev(bo.distinct_batch(B, (Cout,), 11), dtype)
        f = lambda a, t: ops.conv2x2_const_norm_act(a, w, bias, t, Cout, gamma, beta, G, 1e-5)
        relations("conv2x2_const_norm_act temb rows", f, (a, temb), 16)
    else:
        temb = rand_v(Cout, 4).to(dtype)
        f = lambda a: ops.conv2x2_const_norm_act(a, w, bias, temb, 0, gamma, beta, G, 1e-5)
        relations("conv2x2_const_norm_act temb broadcast", f, a, 16)


# ----------------------------------------------------------------------------------------------- conv3h.hip
def _variant(ops, x, w, bias, **kw):
    """(variant id, K slices) of the plan conv2d runs for this call, given the workspace it asks for."""
    kw = {k: v for k, v in kw.items() if k in ("temb", "temb_stride", "residual")}
    probe = ops.conv_args(x, w, bias, out=torch.empty(tuple(x.shape[:-1]) + (w.shape[0],), dtype=x.dtype, device=x.device), **kw)
    need = ops.lib.afldm_conv2d_workspace(ctypes.byref(probe))
    if need:
        ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
        probe.workspace, probe.workspace_bytes = ops.ptr(ws), need
    code = ops.lib.afldm_conv2d_variant(ctypes.byref(probe))
    return (code, 1) if code < 0 else (code & 255, (code >> 8) & 255)


# The halo-patch tiles that hold several whole planes (the variant rows kH3[] of conv3h.hip; BM pixels per tile, NSEG = BM / (N N)
# planes, launch_h3):
#   variant 52: BM 64, 4x4 planes  -> g = 4      variant 68: BM 128, 4x4 planes -> g = 8      variant 67: BM 128, 8x8 -> g = 2
# (51: one 8x8 plane per tile, g = 1 - its tiles cannot mix samples, it runs as the no-variant default below.)  A tile needs
# M % BM == 0 (conv3h_supported, conv3h.hip): at B = g + 1 and 2 g + 1 the planner falls back to the GEMM tiles, which
# run over rows of different samples too, so every form runs at g + 1, 2 g + 1 AND 2 g, 3 g; at the multiples the forced
# variant must be the one that ran.  fp32 takes several samples per tile only as split-K slabs (conv3h_supported).
H3_MULTI = [
    # variant, N, Cin, Cout, K slices (0: the planner's), g
    (52, 4, 256, 192, 1, 4),          # no split: per-sample time embedding, residual, GroupNorm records from the epilogue
    (52, 4, 256, 192, 2, 4),          # split-K
    (68, 4, 256, 96, 1, 8),
    (67, 8, 128, 96, 1, 2),
    (0, 4, 256, 96, 0, 4),            # nothing forced: (4, 4, 4, 256, 96) of H3_CASES
    (0, 8, 384, 96, 0, 2),            # nothing forced, 8x8
]


def _h3_batches(g, forced):
    return sorted({g + 1, 2 * g + 1, 2 * g, 3 * g} | (set() if forced else {64}))       # 64: the planner's choice at the benchmark's batch


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", H3_MULTI, ids=_id)
def test_conv3x3_halo_patch_tiles_of_several_samples(dtype, case):
    """conv2d 3x3 with a time-embedding row per sample, residual and want_stats on the tiles that hold several planes."""
    from afldm_amd import _lib
    ops = _ops()
    v, N, Cin, Cout, sk, g = case
    w, bias = rand_w((Cout, 3, 3, Cin), 9 * Cin, v + N, dtype), rand_v(Cout, 5)
    f = lambda x, t, r: ops.conv2d(x, w, bias, temb=t, temb_stride=Cout, residual=r, want_stats=True)
    ran = []
    try:
        if v:
            _lib.check(_lib.lib.afldm_conv2d_tune(v, sk), "tune")
        for B in _h3_batches(g, v):
            x = dev(bo.distinct_batch(B, (N, N, Cin), 20 + B), dtype)
            temb = dev(bo.distinct_batch(B, (Cout,), 21 + B), dtype)
            res = dev(bo.distinct_batch(B, (N, N, Cout), 22 + B), dtype)
            ran.append((B,) + _variant(ops, x, w, bias, temb=temb, temb_stride=Cout, residual=res))
            relations(f"afldm_conv2d halo-patch {case}", f, (x, temb, res), g)
    finally:
        _lib.lib.afldm_conv2d_tune(-1, -1)
    print(f"[halo-patch {_id(dtype)} {case}] (B, variant, K slices): {ran}")
    if v and (dtype == BF16 or sk > 1):
        for B, got, z in ran:
            if B % g == 0:
                assert got == v and (z == sk), f"variant {v} x {sk} did not run at B={B}: {got} x {z}"


@pytest.mark.parametrize("B", [8, 12, 9, 64])
def test_conv3x3_halo_patch_folded_shortcut(B):
    """conv2d with the folded 1x1 shortcut at the smallest 4x4 site (FOLD3_SITES: 384 | 0 -> 768, bf16; g = 4 or 8 planes per
    tile): B = 8, 12 (whole tiles), 9 (where conv2d_shortcut_ok allows it) and 64 (the plan of the benchmark, K split)."""
    ops = _ops()
    N, C1, Cout, dtype = 4, 384, 768, BF16
    w2, wsc = rand_w((Cout, 3, 3, Cout), 9 * Cout, 31, dtype), rand_w((Cout, 1, 1, C1), C1, 32, dtype)
    bias = rand_v(Cout, 33)
    h = dev(bo.distinct_batch(B, (N, N, Cout), 34), dtype)
    x1 = dev(bo.distinct_batch(B, (N, N, C1), 35), dtype)
    ok = ops.conv2d_shortcut_ok(h, w2, bias, (x1, None, wsc))
    print(f"[folded shortcut B={B}] conv2d_shortcut_ok = {ok}")
    if B in (8, 64):
        assert ok == 2, "the 4x4 site folds its shortcut on a three-tap tile at batch 8 and 64"
    if not ok:
        with pytest.raises(Exception, match="folded shortcut"):
            ops.conv2d(h, w2, bias, want_stats=True, shortcut=(x1, None, wsc))
        return
    f = lambda h, x1: ops.conv2d(h, w2, bias, want_stats=True, shortcut=(x1, None, wsc))
    relations("afldm_conv2d folded shortcut", f, (h, x1), 4)
    relations("afldm_conv2d folded shortcut", f, (h, x1), 8, rotations=())


@pytest.mark.parametrize("N,C,B", [(8, 384, 3), (8, 384, 9), (8, 384, 64), (4, 384, 8), (4, 384, 12), (4, 384, 64)], ids=_id)
def test_conv3x3_norm_out_epilogue(N, C, B):
    """conv2d(..., norm_out=...): the GroupNorm that follows, applied by the epilogue where a tile holds whole samples
    (afldm_conv2d_norm_ok) - `.norm_applied` is one more output when the plan gives it."""
    ops = _ops()
    dtype, G = BF16, 32
    w, bias = rand_w((C, 3, 3, C), 9 * C, 41, dtype), rand_v(C, 42)
    gamma, beta = rand_v(C, 43, 0.1, 1.0), rand_v(C, 44, 0.1)
    seen = []

    def f(x, t):
        y = ops.conv2d(x, w, bias, temb=t, temb_stride=C, want_stats=True, norm_out=(gamma, beta, G, 1e-5))
        hn = getattr(y, "norm_applied", None)
        seen.append(hn is not None)
        return y if hn is None else (y, hn)
    x = dev(bo.distinct_batch(B, (N, N, C), 45), dtype)
    temb = dev(bo.distinct_batch(B, (C,), 46), dtype)
    relations(f"afldm_conv2d norm_out N={N}", f, (x, temb), 2 if N == 8 else 4)
    print(f"[norm_out N={N} B={B}] epilogue normalised: {seen[0]}")
    assert len(set(seen)) == 1
    if N == 8 and B == 64:
        assert seen[0], "the one-sample 8x8 tile normalises in its epilogue at batch 64"


# ----------------------------------------------------------------------------------------------- 1x1 / dense layers
# skinny.hip: 64-row blocks (skinny.hip:219: a block holds whole samples, 64 % HW == 0): 2x2 planes -> g = 16; the 2x2 plane
# as ONE dense layer (blocks.conv_forward: a row is a sample) -> g = 64.
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("B", [17, 33])
def test_conv1x1_skinny_on_2x2_planes(dtype, B):
    ops = _ops()
    C1, C2, Cout = 256, 256, 96               # (K a multiple of 8 MFMA steps on both sides of the seam)
    w, bias = rand_w((Cout, 1, 1, C1 + C2), C1 + C2, 51, dtype), rand_v(Cout, 52)
    x1 = dev(bo.distinct_batch(B, (2, 2, C1), 53), dtype)
    x2 = dev(bo.distinct_batch(B, (2, 2, C2), 54), dtype)
    temb = dev(bo.distinct_batch(B, (Cout,), 55), dtype)
    res = dev(bo.distinct_batch(B, (2, 2, Cout), 56), dtype)
    probe = ops.conv_args(x1, w, bias, x2, temb, Cout, res, torch.empty(B, 2, 2, Cout, device="cuda", dtype=dtype))
    assert ops.lib.afldm_conv2d_variant(ctypes.byref(probe)) == -16, "the skinny kernel does not take this shape"
    f = lambda x1, x2, t, r: ops.conv2d(x1, w, bias, x2=x2, temb=t, temb_stride=Cout, residual=r, want_stats=True)
    relations("afldm_conv2d skinny 2x2", f, (x1, x2, temb, res), 16)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("B", [65, 129])
def test_conv3x3_on_2x2_plane_as_one_dense_layer(dtype, B):
    from afldm_amd.models import blocks
    C1, C2, Cout = 64, 32, 64
    conv = torch.nn.Conv2d(C1 + C2, Cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(conv.weight.shape, generator=torch.Generator().manual_seed(61)) / (3 * (C1 + C2) ** 0.5)).to(dtype))
    conv = conv.cuda()
    x1 = dev(bo.distinct_batch(B, (2, 2, C1), 62), dtype)
    x2 = dev(bo.distinct_batch(B, (2, 2, C2), 63), dtype)
    temb = dev(bo.distinct_batch(B, (Cout,), 64), dtype)
    res = dev(bo.distinct_batch(B, (2, 2, Cout), 65), dtype)
    f = lambda x1, x2, t, r: blocks.conv_forward(conv, (x1, x2), temb=t, temb_stride=Cout, residual=r, want_stats=True)
    relations("afldm_conv2d dense 2x2", f, (x1, x2, temb, res), 64)
    assert ("dense2x2", dtype, C1, C2) in conv.__dict__["_afldm_cache"]


# linear_split (the fused q | k | v projection): GEMM tiles of 64 / 128 token rows (the variant rows of conv.hip) run over the rows
# of several samples: T = 16 -> g = 4 .. 8, T = 64 -> g = 1 .. 2; from M = B T >= 4096 rows the weights-in-registers kernel (lin.hip,
# persistent workgroups over 128-row blocks) takes over: B = 256 / 64 is that switch.
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("T,B,g", [(16, 5, 4), (16, 9, 8), (16, 17, 8), (16, 256, 8), (64, 2, 1), (64, 3, 2), (64, 5, 2), (64, 64, 2)], ids=_id)
def test_linear_split(dtype, T, B, g):
    ops = _ops()
    C = 192
    w, bias = rand_w((3 * C, 1, 1, C), C, 71, dtype), rand_v(3 * C, 72)
    x = dev(bo.distinct_batch(B, (T, C), 73), dtype)
    relations(f"afldm_conv2d linear_split T={T}", lambda x: ops.linear_split(x, w, bias, 2 * C), x, g)


# conv2d_slabs -> af_act_slabs: the split-K slabs come from GEMM tiles of 64 - 256 rows (the variant rows of conv.hip: 16 - 64
# planes of 2x2, 4 - 16 of 4x4); k_af_act_slabs itself takes one sample x `gpb` whole groups per workgroup (af.hip:1616-1619,
# g = 1) and indexes slabs, time embedding and residual by sample  ->  the producer's g = 4 .. 32, one pair of batches per g.
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("N,act", [(2, True), (2, 2), (2, False), (4, True), (4, False)], ids=_id)
def test_conv2d_slabs_finished_by_af_act_slabs(dtype, N, act):
    ops = _ops()
    C, G = 256, 32
    w, bias = rand_w((C, 3, 3, C), 9 * C, 81, dtype), rand_v(C, 82)
    gamma, beta = rand_v(C, 83, 0.1, 1.0), rand_v(C, 84, 0.1)

    def f(x, t, r):
        got = ops.conv2d_slabs(x, w)
        assert got is not None, "the plan of this shape does not split K"
        slabs, nslab = got
        return ops.af_act_slabs(slabs, nslab, bias, t, C, gamma, beta, G, 1e-5, x.shape[0], N, C, dtype,
                                residual=None if act else r, want_raw=True, act=act)
    for g in (4, 8, 16, 32):
        for B in (g + 1, 2 * g + 1):
            x = dev(bo.distinct_batch(B, (N, N, C), 85 + B), dtype)
            temb = dev(bo.distinct_batch(B, (C,), 86 + B), dtype)
            res = dev(bo.distinct_batch(B, (N, N, C), 87 + B), dtype)
            relations(f"conv2d_slabs + af_act_slabs N={N} act={act}", f, (x, temb, res), g)


# resconv.hip: kBM = 128 output rows per tile (resconv.hip:37), a tile holds BM / plane whole samples (resconv.hip:243).
# Smallest sites: s2 8x8 -> 4x4 (16 rows a sample, g = 8); up2 4x4 -> 8x8 (its GEMM rows are the 16 INPUT pixels, g = 8).
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("B", [9, 17])
@pytest.mark.parametrize("form", ["s2", "up2"])
def test_resampling_convolutions(dtype, form, B):
    ops = _ops()
    Cin, Cout = 64, 64
    bias = rand_v(Cout, 91)
    wf = torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(92)) / (3 * Cin ** 0.5)
    if form == "s2":
        w = ops.pack_weight(wf.cuda(), dtype)
        x = dev(bo.distinct_batch(B, (8, 8, Cin), 93), dtype)
        f = lambda x: ops.conv2d_s2(x, w, bias, pad=(1, 1), want_stats=True)
    else:
        w = ops.pack_weight_up2(wf.cuda(), dtype)
        x = dev(bo.distinct_batch(B, (4, 4, Cin), 94), dtype)
        f = lambda x: ops.conv2d_up2(x, w, bias, want_stats=True)
    relations(f"afldm_conv2d_{form}", f, x, 8)


# ----------------------------------------------------------------------------------------------- GroupNorm
# gn.hip: k_gn_partial runs B x S workgroups (gn.hip:279) and k_gn_apply B x ceil(HW / rows) with rows <= HW (gn.hip:300-303):
# no workgroup spans two samples, g = 1  ->  B = 2, 3.
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("HW", [4, 16, 64])
@pytest.mark.parametrize("B", [2, 3])
def test_gn_stats_and_apply(dtype, HW, B):
    ops = _ops()
    C1, C2, G = 96, 48, 8
    side = int(HW ** 0.5)
    gamma, beta = rand_v(C1 + C2, 101, 0.2, 1.0), rand_v(C1 + C2, 102, 0.3)
    x1 = dev(bo.distinct_batch(B, (side, side, C1), 103), dtype)
    x2 = dev(bo.distinct_batch(B, (side, side, C2), 104), dtype)

    def f(x1, x2):
        st = ops.gn_stats(x1, G, x2=x2)
        return (ops.gn_apply(x1, st, gamma, beta, G, 1e-5, act=1, x2=x2), st.st1, st.st2)
    relations("afldm_gn_stats + afldm_gn_apply concat", f, (x1, x2), 1)
    one = lambda x: ops.gn_apply(x, ops.gn_stats(x, G), gamma[:C1].contiguous(), beta[:C1].contiguous(), G, 1e-5)
    relations("afldm_gn_stats + afldm_gn_apply", one, x1, 1)


# ----------------------------------------------------------------------------------------------- alias-free activation
# k_af_act_small: one THREAD per (sample, channel) plane, 256 threads a workgroup (af.hip:753-762), the 64 lanes of a wave
# work out their GroupNorm keys together (gn_wave_keys): with 48 channels a workgroup holds 5 1/3 samples and every wave
# straddles two  ->  g = 5 (B = 6, 11; 7 and 12 put the seams elsewhere).  N = 8 with 16-channel items: k_af_act_kron / p8 take
# 4 items of 16 channels per workgroup (af.hip:512, :1344): 3 items a sample -> 1 1/3 samples per workgroup.
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("N", [2, 4, 8])
@pytest.mark.parametrize("B", [6, 7, 11, 12])
def test_af_act_small_planes(dtype, N, B):
    ops = _ops()
    C1, C2, G = 32, 16, 8
    gamma, beta = rand_v(C1 + C2, 111, 0.2, 1.0), rand_v(C1 + C2, 112, 0.3)
    x1 = dev(bo.distinct_batch(B, (N, N, C1), 113), dtype)
    x2 = dev(bo.distinct_batch(B, (N, N, C2), 114), dtype)
    f = lambda x1, x2: ops.af_act(x1, x2, ops.gn_stats(x1, G, x2=x2), gamma, beta, G, 1e-5)
    print(f"[af_act N={N} B={B} {_id(dtype)}] route {ops.af_act_route(dtype, N, C1, C2, B)}")
    relations(f"afldm_af_act N={N}", f, (x1, x2), 5)
    relations(f"afldm_af_act N={N} no norm", lambda x: ops.af_act(x), x1, 5)
    if N == 2:
        c2 = lambda x1, x2: ops.af_act(x1, x2, ops.gn_stats(x1, G, x2=x2), gamma, beta, G, 1e-5, out_const=True)
        relations("afldm_af_act_const2", c2, (x1, x2), 5)
    if N == 8:
        with ops.af_tune(small_n=12):
            assert ops.af_act_route(dtype, N, C1, C2, B).kernel == "small"
            relations("afldm_af_act N=8 small", f, (x1, x2), 5)


# k_af_act_plane walks a contiguous range of ipw = ceil(items / grid) (sample, channel block) items per workgroup (af.hip:138-
# 142); max_grid = 2 makes that range 1 1/2 samples at B = 3 and 2 1/2 at B = 5 (4 items of 8 channels a sample)  ->  g = 1, 2.
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("N", [16, 32])
@pytest.mark.parametrize("B", [3, 5])
def test_af_act_plane_kernel_walking_several_items(dtype, N, B):
    ops = _ops()
    C, G = 32, 8
    gamma, beta = rand_v(C, 121, 0.2, 1.0), rand_v(C, 122, 0.3)
    x = dev(bo.distinct_batch(B, (N, N, C), 123), dtype)
    f = lambda x: ops.af_act(x, None, ops.gn_stats(x, G), gamma, beta, G, 1e-5)
    with ops.af_tune(ch=8, max_grid=2):
        r = ops.af_act_route(dtype, N, C, 0, B)
        assert r.kernel == "plane" and r.grid == 2 and r.items_per_wg == 2 * B, r
        relations(f"afldm_af_act plane N={N}", f, x, B // 2 + 1)
    assert ops.af_act_route(dtype, N, C, 0, B).grid != 2, "af_tune restores the planner"


# The resamplers: k_resample_plane strides (sample, 16-channel) items over the grid (af.hip:1134), the small / reg routes of
# afldm_af_resample contract one axis over rows of the flattened tensor: C = 48 gives 3 items a sample  ->  B = 3, 9.
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("op,N", [("up2", 4), ("up2", 8), ("up2", 16), ("down2", 4), ("down2", 8), ("down2", 32)], ids=_id)
@pytest.mark.parametrize("B", [3, 9])
def test_af_resamplers(dtype, op, N, B):
    ops = _ops()
    x = dev(bo.distinct_batch(B, (N, N, 48), 131), dtype)
    f = (lambda x: ops.af_up2(x)) if op == "up2" else (lambda x: ops.af_lpf_down2(x, want_stats=True))
    relations(f"af_{op} N={N}", f, x, 2)


# ----------------------------------------------------------------------------------------------- attention
# afldm_attention: a workgroup is the query block(s) of ONE (sample, head) (attn.hip:10, grid = B heads qblocks)  ->  g = 1; from
# B heads >= 1024 pairs the small planes take 2- / 1-wave workgroups (attn_waves, attn.hip:615-624): B = 32 at 32 heads.
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("T", [4, 16, 64])
@pytest.mark.parametrize("B", [2, 3, 32, 33])
def test_attention(dtype, T, B):
    ops = _ops()
    heads, d = 32, 24
    C = heads * d
    q, k, v = (dev(bo.distinct_batch(B, (T, C), 141 + i), dtype) for i in range(3))
    f = lambda q, k, v: ops.attention(q, k, v.transpose(1, 2).contiguous(), heads)
    relations(f"afldm_attention T={T}", f, (q, k, v), 1)


def _attn_block(T, C, d, G, B, seed):
    ops = _ops()
    side = int(T ** 0.5)
    x = dev(bo.distinct_batch(B, (T, C), seed), BF16)
    gamma, beta = rand_v(C, seed + 1, 0.2, 1.0), rand_v(C, seed + 2, 0.3)
    wq, bq = rand_w((3 * C, 1, 1, C), C, seed + 3, BF16), rand_v(3 * C, seed + 4, 0.2)
    wo, bo_ = rand_w((C, 1, 1, C), C, seed + 5, BF16), rand_v(C, seed + 6, 0.2)
    stats = lambda x: ops.gn_stats(x.view(x.shape[0], side, side, C), G)
    return x, gamma, beta, wq, bq, wo, bo_, stats


# afldm_attn_block_fused: grid = B heads, one workgroup per (sample, head) (attnf.hip:740)  ->  g = 1; B = 3, 9.
@pytest.mark.parametrize("T,C,d,G", [(1024, 192, 24, 32), (256, 384, 24, 32), (256, 64, 16, 8), (64, 128, 16, 8)], ids=_id)
@pytest.mark.parametrize("B", [3, 9])
def test_attn_block_fused(T, C, d, G, B):
    ops = _ops()
    assert ops.lib.afldm_attn_block_fused_supported(T, C, d, G)
    x, gamma, beta, wq, bq, _, _, stats = _attn_block(T, C, d, G, B, 151)
    f = lambda x: ops.attn_block_fused(x, stats(x), gamma, beta, G, 1e-5, wq, bq, C // d, d ** -0.5)
    relations(f"afldm_attn_block_fused T={T} C={C}", f, x, 1)


# afldm_attn_identity_block: BM token rows per workgroup (pag.hip:374-378: 128 at C <= 192, 64 at 384, 32 at 768) over the
# B T rows  ->  g = BM / T.  The policy (ops._IDENTITY_MIN_T) sends T >= 1024 to it: there a tile lies inside one sample (g = 1);
# the small levels, where tiles hold several samples, run with the policy lowered as tests/test_gpu_pag.py does.
@pytest.mark.parametrize("T,C,g", [(1024, 192, 1), (64, 64, 2), (16, 64, 8), (4, 64, 32), (4, 768, 8)], ids=_id)
def test_attn_identity_block(T, C, g, monkeypatch):
    ops = _ops()
    G = 32
    if T < 1024:
        monkeypatch.setattr(ops, "_IDENTITY_MIN_T", 4)
    gamma, beta = rand_v(C, 161, 0.2, 1.0), rand_v(C, 162, 0.3)
    w, bias = rand_w((C, 1, 1, C), C, 163, BF16), rand_v(C, 164, 0.1)
    f = lambda x: ops.attn_identity_block(x, ops.gn_stats(x, G), gamma, beta, G, 1e-5, w, bias)
    for B in (g + 1, 2 * g + 1):
        x = dev(bo.distinct_batch(B, (T, C), 165 + B), BF16)
        assert ops.attn_identity_block_ok(x, G)
        relations(f"afldm_attn_identity_block T={T} C={C}", f, x, g)


# afldm_attn_block_fused_out: the eight head workgroups of a sample hand over inside one XCD; work ids are dealt to the 8 XCDs
# in equal contiguous runs (attnf.hip:778-784: B % 8 == 0)  ->  B / 8 samples per XCD: B = 8, 16, 24 give 1, 2, 3.
@pytest.mark.parametrize("B", [8, 16, 24])
def test_attn_block_fused_out(B):
    ops = _ops()
    T, C, d, G = 1024, 192, 24, 32
    x, gamma, beta, wq, bq, wo, bo_, stats = _attn_block(T, C, d, G, B, 171)
    if not ops.attn_block_fused_out_ok(x, C // d, G):
        pytest.skip("no in-launch hand-over on this device (partitioned or masked)")
    sync = ops.new_sync_buffer(x.device)
    f = lambda x: ops.attn_block_fused_out(x, stats(x), gamma, beta, G, 1e-5, wq, bq, C // d, d ** -0.5, wo, bo_)
    with ops.sync_scope(sync):
        relations("afldm_attn_block_fused_out", f, x, B // 8)
    torch.cuda.synchronize()
    assert int(sync.abs().sum().item()) == 0, "hand-over counters / error word must be back at zero"


def test_wall_time_of_this_file():
    """(Printed for the record: the module's wall time up to here, model builds included.)"""
    print(f"[batch positions] wall time of the file: {time.time() - _T0[0]:.1f} s")
