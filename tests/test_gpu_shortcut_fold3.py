"""GPU tests: the ResnetBlock2D 1x1 conv_shortcut folded into conv2 on the halo-patch tiles that take THREE filter taps per K step
(the 8x8 / 4x4 planes, split-K slabs included, and the small batches) - afldm_conv2d_shortcut_ok == 2, blocks._SC_FOLD3 - against
the two launches it replaces.  Tolerances: those of tests/test_gpu_shortcut_fold.py (same error class: one rounding fewer, another
summation order)."""
import ctypes

import pytest
import torch

from test_gpu_r02 import build_unet, rel_rms
from test_gpu_shortcut_fold import _CountConv, _block, _operands, _plan_folds, _ref64

pytestmark = pytest.mark.gpu

# (plane, shortcut input channels C1 | C2, Cout): the 8^2 / 4^2 sites of the FFHQ UNet whose blocks change their width
SITES = [(8, 768, 384, 384), (8, 384, 384, 384), (4, 768, 768, 768), (4, 768, 384, 768), (4, 384, 0, 768)]
# batch 64, plus one small batch per tile family: one- and two-sample tiles at 8^2 (B = 2 / 3: an odd count), four / eight at 4^2
BATCHES = {8: (64, 2, 3), 4: (64, 8, 4)}
# Site classes turned off in shortcut_ok (csrc/conv.hip) after the in-step measurement: none.
CLASSES_OFF = ()


def _packed(B, N, C1, C2, Cout, dtype, seed):
    from afldm_amd import ops
    h, x1, x2, w2, wsc, b2, bsc = _operands(B, N, C1, C2, Cout, dtype, seed)
    pw2, pwsc = ops.pack_weight(w2, dtype), ops.pack_weight(wsc, dtype)
    bias = (b2.double() + bsc.double()).float().contiguous()
    return h, x1, x2, w2, wsc, b2, bsc, pw2, pwsc, bias


def _splitk(h, pw2):
    """K slices of the plan that conv2d(h, pw2) runs (given the workspace it asks for)."""
    from afldm_amd import ops
    a = ops.conv_args(h, pw2, None, None, out=h)
    need = ops.lib.afldm_conv2d_workspace(ctypes.byref(a))
    if need:
        a.workspace, a.workspace_bytes = ops.ptr(h), need
    code = ops.lib.afldm_conv2d_variant(ctypes.byref(a))
    assert code >= 0
    return (code >> 8) & 255


def _compare(dtype, got, ref, y64=None):
    """bf16: rel-RMS against the two-launch form; fp32: both against an fp64 evaluation (relative max-abs)."""
    if dtype == torch.float32:
        scale = float(y64.abs().max())
        e_fold, e_two = (float((t.double() - y64).abs().max()) / scale for t in (got, ref))
        print(f"[fold3 fp32] e_fold {e_fold:.3e} e_two {e_two:.3e}")
        assert e_fold <= max(2e-6, 1.25 * e_two), (e_fold, e_two)
    else:
        err = rel_rms(got, ref.cpu())
        print(f"[fold3 bf16] rel-RMS {err:.3e}")
        assert err <= 4e-3, err


def _fold_vs_two(dtype, B, N, C1, C2, Cout, need_ok):
    from afldm_amd import ops
    h, x1, x2, w2, wsc, b2, bsc, pw2, pwsc, bias = _packed(B, N, C1, C2, Cout, dtype, B * 1000 + N + C1 + C2)
    sc = (x1, x2, pwsc)
    ok = ops.conv2d_shortcut_ok(h, pw2, bias, sc)
    if need_ok:
        assert ok == 2, "this site takes the folded shortcut on a three-tap tile"
    if not ok:
        with pytest.raises(Exception, match="folded shortcut"):
            ops.conv2d(h, pw2, bias, want_stats=True, shortcut=sc)
        return None
    res = ops.conv2d(x1, pwsc, bsc, x2=x2)
    ref = ops.conv2d(h, pw2, b2, residual=res, want_stats=True)
    got = ops.conv2d(h, pw2, bias, want_stats=True, shortcut=sc)
    again = ops.conv2d(h, pw2, bias, want_stats=True, shortcut=sc)
    torch.cuda.synchronize()
    assert torch.equal(got, again) and torch.equal(got.gn_partial, again.gn_partial), "reruns are bit-identical"
    _compare(dtype, got, ref, _ref64(h, w2, b2, x1, x2, wsc, bsc) if dtype == torch.float32 else None)
    # the statistics describe the stored output
    s = got.gn_partial.double().sum(1)
    assert torch.allclose(s[..., 0], got.double().sum((1, 2)), rtol=1e-4, atol=1e-2)
    assert torch.allclose(s[..., 1], got.double().pow(2).sum((1, 2)), rtol=1e-3, atol=1e-2)
    return h, pw2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,C1,C2,Cout,B", [s + (b,) for s in SITES for b in BATCHES[s[0]]])
def test_conv2d_shortcut_fold3_vs_two_launches(dtype, N, C1, C2, Cout, B):
    _fold_vs_two(dtype, B, N, C1, C2, Cout, need_ok=(B == 64 and not CLASSES_OFF))


# 4x4 planes at batch 64, 384 couts: the plan splits K into 3 (bf16, six 64-channel blocks) / 4 (fp32, twelve 32-channel blocks) slices
@pytest.mark.parametrize("dtype,C1,C2,what", [
    (torch.bfloat16, 128, 64, "boundary"),       # the issue's example: 3 shortcut blocks; x1 | x2 meet between the last two slices
    (torch.bfloat16, 128, 128, "uneven"),        # 4 blocks over 3 slices: 1 / 1 / 2
    (torch.bfloat16, 128, 128, "boundary"),      # ... and x1 | x2 meet where the last slice begins
    (torch.float32, 96, 64, "uneven"),           # 5 blocks over 4 slices: 1 / 1 / 1 / 2
    (torch.float32, 64, 64, "boundary"),         # 4 blocks, one per slice
])
def test_conv2d_shortcut_fold3_splitk_shares(dtype, C1, C2, what):
    """Slice ks of z takes the shortcut blocks [nsc ks / z, nsc (ks + 1) / z): shares that differ, and an sc_x1 | sc_x2 boundary
    that falls between two slices."""
    got = _fold_vs_two(dtype, 64, 4, C1, C2, 384, need_ok=True)
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


def test_conv2d_shortcut_fold3_refused():
    """Where afldm_conv2d_shortcut_ok says no, the call raises: a residual beside the shortcut, and a shortcut whose first input
    ends inside a 128-byte channel block."""
    from afldm_amd import ops
    h, x1, x2, w2, wsc, b2, bsc, pw2, pwsc, bias = _packed(64, 8, 384, 384, 384, torch.bfloat16, 1)
    assert ops.conv2d_shortcut_ok(h, pw2, bias, (x1, x2, pwsc)) == 2
    with pytest.raises(Exception, match="folded shortcut"):
        ops.conv2d(h, pw2, bias, residual=h, want_stats=True, shortcut=(x1, x2, pwsc))
    h, x1, x2, w2, wsc, b2, bsc, pw2, pwsc, bias = _packed(64, 8, 96, 32, 384, torch.bfloat16, 2)
    assert not ops.conv2d_shortcut_ok(h, pw2, bias, (x1, x2, pwsc))
    with pytest.raises(Exception, match="folded shortcut"):
        ops.conv2d(h, pw2, bias, want_stats=True, shortcut=(x1, x2, pwsc))
    # a plan that does not split K has no slabs to hand over
    h, x1, x2, w2, wsc, b2, bsc, pw2, pwsc, bias = _packed(64, 8, 384, 0, 384, torch.bfloat16, 3)
    assert not ops.conv2d_shortcut_ok(h, pw2, None, (x1, x2, pwsc), slabs=True)


def _gn64(y64, gamma, beta, G, eps):
    B, N, _, C = y64.shape
    v = y64.reshape(B, N * N, G, C // G)
    mean, var = v.mean((1, 3), keepdim=True), v.var((1, 3), unbiased=False, keepdim=True)
    return ((v - mean) / (var + eps).sqrt()).reshape(B, N, N, C) * gamma.double() + beta.double()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,C1,C2,Cout", [s for s in SITES if s[0] == 4])
def test_slabs_shortcut_fold3_into_next_norm(dtype, N, C1, C2, Cout):
    """conv2 as split-K slabs carrying the folded shortcut, finished by af_act_slabs(act=False) with the bias b2 + b_sc and no
    residual - against plain slabs + the separate 1x1 launch as the residual.  Both returned tensors: raw and normalised."""
    from afldm_amd import ops
    B, G, eps = 64, 32, 1e-5
    h, x1, x2, w2, wsc, b2, bsc, pw2, pwsc, bias = _packed(B, N, C1, C2, Cout, dtype, 77 + C1 + C2)
    g = torch.Generator().manual_seed(C1)
    gamma, beta = (1.0 + 0.1 * torch.randn(Cout, generator=g)).cuda(), (0.1 * torch.randn(Cout, generator=g)).cuda()
    sc = (x1, x2, pwsc)
    assert ops.conv2d_shortcut_ok(h, pw2, None, sc, slabs=True) == 2
    res = ops.conv2d(x1, pwsc, bsc, x2=x2)
    slabs, nslab = ops.conv2d_slabs(h, pw2)
    hn_ref, y_ref = ops.af_act_slabs(slabs, nslab, b2.float().contiguous(), None, 0, gamma, beta, G, eps, B, N, Cout, dtype,
                                     residual=res, want_raw=True, act=False)
    outs = []
    for _ in range(2):
        slabs, nslab2 = ops.conv2d_slabs(h, pw2, shortcut=sc)
        assert nslab2 == nslab
        outs.append(ops.af_act_slabs(slabs, nslab2, bias, None, 0, gamma, beta, G, eps, B, N, Cout, dtype, want_raw=True, act=False))
    torch.cuda.synchronize()
    (hn, y), (hn2, y2) = outs
    assert torch.equal(hn, hn2) and torch.equal(y, y2), "reruns are bit-identical"
    y64 = _ref64(h, w2, b2, x1, x2, wsc, bsc) if dtype == torch.float32 else None
    _compare(dtype, y, y_ref, y64)
    _compare(dtype, hn, hn_ref, _gn64(y64, gamma, beta, G, eps) if dtype == torch.float32 else None)


@pytest.mark.parametrize("C1,C2,Cout", [s[1:] for s in SITES if s[0] == 8])
def test_norm_out_epilogue_with_fold3(C1, C2, Cout):
    """8x8 planes (bf16, one sample per tile): the epilogue applies the GroupNorm that follows to the folded output."""
    from afldm_amd import ops
    B, N, G, eps, dtype = 64, 8, 32, 1e-5, torch.bfloat16
    h, x1, x2, w2, wsc, b2, bsc, pw2, pwsc, bias = _packed(B, N, C1, C2, Cout, dtype, 5 + C1)
    g = torch.Generator().manual_seed(C1)
    gamma, beta = (1.0 + 0.1 * torch.randn(Cout, generator=g)).cuda(), (0.1 * torch.randn(Cout, generator=g)).cuda()
    out = ops.conv2d(h, pw2, bias, want_stats=True, shortcut=(x1, x2, pwsc), norm_out=(gamma, beta, G, eps))
    plain = ops.conv2d(h, pw2, bias, want_stats=True, shortcut=(x1, x2, pwsc))
    hn = getattr(out, "norm_applied", None)
    assert hn is not None, "the one-sample 8x8 tile normalises in its epilogue"
    assert torch.equal(out, plain) and torch.equal(out.gn_partial, plain.gn_partial)
    want = ops.gn_apply(out, ops.gn_stats(out), gamma, beta, G, eps)       # (the statistics the epilogue attached)
    torch.cuda.synchronize()
    err = rel_rms(hn, want.cpu())
    print(f"[fold3 norm_out] rel-RMS {err:.3e}")
    assert err <= 4e-3, err


# (fp32: relative max-abs, bf16: rel-RMS - as test_resnet_block_shortcut_fold_switch)
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 4e-3)])
@pytest.mark.parametrize("B", [64, 8])
@pytest.mark.parametrize("N,C1,C2,Cout", SITES)
def test_resnet_block_shortcut_fold3_switch(monkeypatch, dtype, tol, B, N, C1, C2, Cout):
    """ResnetBlock2D forward with the three-tap fold on and off (AFLDM_NO_SHORTCUT_FOLD3): same result within the tolerances, one
    afldm_conv2d call fewer with it on - wherever the plan of this (batch, dtype) puts conv2 on a three-tap halo-patch tile."""
    from afldm_amd import ops
    from afldm_amd.models import blocks
    blk = _block(C1 + C2, Cout, dtype)
    g = torch.Generator().manual_seed(N + C1)
    x1 = torch.randn(B, N, N, C1, generator=g).cuda().to(dtype)
    x2 = torch.randn(B, N, N, C2, generator=g).cuda().to(dtype) if C2 else None
    inp = (x1, x2) if C2 else x1
    temb = torch.randn(1, Cout, generator=g).cuda().to(dtype)
    w2, _ = blocks.packed_conv(blk.conv2, dtype)
    wsc, _ = blocks.packed_conv(blk.conv_shortcut, dtype)
    folds = ops.conv2d_shortcut_ok(torch.empty(B, N, N, Cout, dtype=dtype, device="cuda"), w2, blk._sc_bias(), (x1, x2, wsc)) == 2
    assert folds or B != 64 or CLASSES_OFF, "the batch-64 sites fold"
    outs, calls = {}, {}
    for fold in (True, False):
        monkeypatch.setattr(blocks, "_SC_FOLD3", fold)
        counter = _CountConv(ops.lib)
        monkeypatch.setattr(ops, "lib", counter)
        y = blk(inp, temb.view(-1), 0)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "lib", counter.raw)
        outs[fold], calls[fold] = y.float().clone(), counter.n
        assert getattr(y, "gn_partial", None) is not None
        assert not _plan_folds(blk, 1), "no one-tap plan on these tiles"
    assert calls[True] == calls[False] - (1 if folds else 0), calls
    if dtype == torch.float32:
        err = float((outs[True].double() - outs[False].double()).abs().max() / outs[False].double().abs().max())
        assert err <= tol, err
    else:
        assert rel_rms(outs[True], outs[False].cpu()) <= tol
    monkeypatch.setattr(blocks, "_SC_FOLD3", True)
    assert torch.equal(blk(inp, temb.view(-1), 0).float(), outs[True]), "reruns with the fold are bit-identical"


def test_unet_forward_fold3_launches_and_graph_replay(monkeypatch):
    """The FFHQ UNet at batch 64 (bf16), toggling _SC_FOLD3 only: seven more blocks lose their conv_shortcut launch (three up-path
    blocks at 8^2, three at 4^2, the 4^2 down block), the output stays within the bf16 budget of the unfolded form, and a graph
    replay of three engine steps is bit-identical to the eager launches."""
    from afldm_amd import ops
    from afldm_amd.engine import DenoiseEngine
    from afldm_amd.models import blocks
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    unet, cfg, _ = build_unet("ffhq", torch.bfloat16)
    B = 64
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, cfg["in_channels"], cfg["sample_size"], cfg["sample_size"], generator=g)
    xb = x.cuda().to(torch.bfloat16)
    folded_blocks, outs, calls = [], {}, {}
    for fold in (False, True):
        monkeypatch.setattr(blocks, "_SC_FOLD3", fold)
        counter = _CountConv(ops.lib)
        monkeypatch.setattr(ops, "lib", counter)
        with torch.no_grad():
            y = unet(xb, 981).sample
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "lib", counter.raw)
        outs[fold], calls[fold] = y.float().clone(), counter.n
        if fold:
            folded_blocks = [m for m in unet.modules() if isinstance(m, blocks.ResnetBlock2D) and _plan_folds(m, 2)]
    assert len(folded_blocks) == 7 - len(CLASSES_OFF), len(folded_blocks)
    assert calls[False] - calls[True] == len(folded_blocks), (calls, len(folded_blocks))
    err = rel_rms(outs[True], outs[False].cpu())
    print(f"[fold3 unet] rel-RMS on / off {err:.3e}")
    assert err <= 2e-2, err
    eng = DenoiseEngine(unet, ffhq_ddim_scheduler(), B, 50, use_graph=True, steps_per_graph=3)
    eng.reset(x)
    eng.step(3)
    graph = eng.lat.clone()
    eager = DenoiseEngine(unet, ffhq_ddim_scheduler(), B, 50, use_graph=False)
    eager.reset(x)
    eager.step(3)
    assert torch.equal(eager.lat, graph), "graph replay must be bit-identical to eager launches"
