"""GPU tests: the ResnetBlock2D 1x1 conv_shortcut folded into conv2 (afldm_conv_args.sc_*, afldm_conv2d_shortcut_ok): extra
centre-tap K steps of the halo-patch kernel over the block input, one bias b2 + b_sc - against the two launches it replaces
(conv1x1 -> conv3x3 with the 1x1 output as residual)."""
import pytest
import torch

from test_gpu_r02 import build_unet, rel_rms

pytestmark = pytest.mark.gpu

# (plane, shortcut input channels C1 | C2, Cout): the halo-patch sites of the FFHQ UNet whose blocks change their width
SITES = [(32, 384, 192, 192), (32, 192, 192, 192), (16, 384, 384, 384), (16, 384, 192, 384), (16, 192, 0, 384)]


def _operands(B, N, C1, C2, Cout, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    h = torch.randn(B, N, N, Cout, generator=g).to(dev, dtype)
    x1 = torch.randn(B, N, N, C1, generator=g).to(dev, dtype)
    x2 = torch.randn(B, N, N, C2, generator=g).to(dev, dtype) if C2 else None
    w2 = torch.randn(Cout, Cout, 3, 3, generator=g) / (3.0 * Cout ** 0.5)
    wsc = torch.randn(Cout, C1 + C2, 1, 1, generator=g) / (C1 + C2) ** 0.5
    b2, bsc = torch.randn(Cout, generator=g) * 0.1, torch.randn(Cout, generator=g) * 0.1
    return h, x1, x2, w2.to(dev), wsc.to(dev), b2.to(dev), bsc.to(dev)


def _ref64(h, w2, b2, x1, x2, wsc, bsc):
    """conv3x3(h, w2) + b2 + conv1x1(x1 | x2, wsc) + bsc in fp64 (NHWC; taps as shifted GEMMs)."""
    B, N, _, C = h.shape
    hp = torch.nn.functional.pad(h.double(), (0, 0, 1, 1, 1, 1))
    w = w2.double()
    y = torch.zeros(B, N, N, w.shape[0], dtype=torch.float64, device=h.device)
    for kh in range(3):
        for kw in range(3):
            y += hp[:, kh:kh + N, kw:kw + N, :] @ w[:, :, kh, kw].t()
    xs = x1.double() if x2 is None else torch.cat([x1.double(), x2.double()], -1)
    return y + xs @ wsc.double()[:, :, 0, 0].t() + b2.double() + bsc.double()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [64, 8, 3, 1])
@pytest.mark.parametrize("N,C1,C2,Cout", SITES)
def test_conv2d_shortcut_fold_vs_two_launches(dtype, B, N, C1, C2, Cout):
    from afldm_amd import ops
    h, x1, x2, w2, wsc, b2, bsc = _operands(B, N, C1, C2, Cout, dtype, B * 1000 + N + C1 + C2)
    pw2, pwsc = ops.pack_weight(w2, dtype), ops.pack_weight(wsc, dtype)
    bias = (b2.double() + bsc.double()).float().contiguous()
    sc = (x1, x2, pwsc)
    ok = ops.conv2d_shortcut_ok(h, pw2, bias, sc)
    if B == 64:
        assert ok, "the batch-64 halo-patch sites take the folded shortcut"
    if not ok:
        with pytest.raises(Exception, match="folded shortcut"):
            ops.conv2d(h, pw2, bias, want_stats=True, shortcut=sc)
        return
    res = ops.conv2d(x1, pwsc, bsc, x2=x2)
    ref = ops.conv2d(h, pw2, b2, residual=res, want_stats=True)
    got = ops.conv2d(h, pw2, bias, want_stats=True, shortcut=sc)
    again = ops.conv2d(h, pw2, bias, want_stats=True, shortcut=sc)
    torch.cuda.synchronize()
    assert torch.equal(got, again) and torch.equal(got.gn_partial, again.gn_partial), "reruns are bit-identical"
    if dtype == torch.float32:
        # both fp32 forms against an fp64 evaluation: the fold is within 2e-6 (relative max-abs) or no worse than the two launches
        y64 = _ref64(h, w2, b2, x1, x2, wsc, bsc)
        scale = float(y64.abs().max())
        e_fold, e_two = (float((t.double() - y64).abs().max()) / scale for t in (got, ref))
        assert e_fold <= max(2e-6, 1.25 * e_two), (e_fold, e_two)
    else:
        assert rel_rms(got, ref.cpu()) <= 4e-3
    # the statistics describe the stored output
    s = got.gn_partial.double().sum(1)
    assert torch.allclose(s[..., 0], got.double().sum((1, 2)), rtol=1e-4, atol=1e-2)


def _block(cin, cout, dtype):
    from afldm_amd.af_modules.af_blocks import WarpedNonlinearity
    from afldm_amd.models import blocks
    torch.manual_seed(5)
    blk = blocks.ResnetBlock2D(in_channels=cin, out_channels=cout, temb_channels=64, groups=32, eps=1e-5)
    blk.nonlinearity = WarpedNonlinearity(blk.nonlinearity)
    return blk.cuda().to(dtype)


def _plan_folds(blk, kind):
    """True when one of the block's cached plans folds the shortcut into conv2 on a tile of this kind (1: one filter tap per K
    step, 2: three)."""
    return any(p.fold == kind for p in blk.__dict__.get("_afldm_plan", {}).values())


class _CountConv:
    """ops.lib with the afldm_conv2d launches counted."""

    def __init__(self, raw):
        self.raw, self.n = raw, 0

    def __getattr__(self, name):
        f = getattr(self.raw, name)
        if name != "afldm_conv2d":
            return f

        def counted(*a):
            self.n += 1
            return f(*a)
        return counted


# (fp32: relative max-abs - the two forms sum in different orders, see test_conv2d_shortcut_fold_vs_two_launches; bf16: rel-RMS)
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 4e-3)])
@pytest.mark.parametrize("N,C1,C2,Cout", SITES)
def test_resnet_block_shortcut_fold_switch(monkeypatch, dtype, tol, N, C1, C2, Cout):
    """ResnetBlock2D forward with the fold on and off (AFLDM_NO_SHORTCUT_FOLD): same result within the tolerances, one
    afldm_conv2d call fewer with it on."""
    from afldm_amd import ops
    from afldm_amd.models import blocks
    B = 64
    blk = _block(C1 + C2, Cout, dtype)
    g = torch.Generator().manual_seed(N + C1)
    x1 = torch.randn(B, N, N, C1, generator=g).cuda().to(dtype)
    x2 = torch.randn(B, N, N, C2, generator=g).cuda().to(dtype) if C2 else None
    inp = (x1, x2) if C2 else x1
    temb = torch.randn(1, Cout, generator=g).cuda().to(dtype)
    outs, calls = {}, {}
    for fold in (True, False):
        monkeypatch.setattr(blocks, "_SC_FOLD", fold)
        counter = _CountConv(ops.lib)
        monkeypatch.setattr(ops, "lib", counter)
        y = blk(inp, temb.view(-1), 0)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "lib", counter.raw)
        outs[fold], calls[fold] = y.float().clone(), counter.n
        assert getattr(y, "gn_partial", None) is not None
    assert calls[True] == calls[False] - 1, calls
    if dtype == torch.float32:
        err = float((outs[True].double() - outs[False].double()).abs().max() / outs[False].double().abs().max())
        assert err <= tol, err
    else:
        assert rel_rms(outs[True], outs[False].cpu()) <= tol
    # reruns with the fold are bit-identical
    monkeypatch.setattr(blocks, "_SC_FOLD", True)
    assert torch.equal(blk(inp, temb.view(-1), 0).float(), outs[True])


def test_unet_forward_launches_without_shortcuts(monkeypatch):
    """The FFHQ UNet at batch 64 (bf16): the folded blocks' conv_shortcut launches are gone from the forward, and the output stays
    within the bf16 budget of the two-launch form."""
    from afldm_amd import ops
    from afldm_amd.models import blocks
    unet, cfg, _ = build_unet("ffhq", torch.bfloat16)
    B = 64
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, cfg["in_channels"], cfg["sample_size"], cfg["sample_size"], generator=g).cuda().to(torch.bfloat16)
    folded_blocks = []
    outs, calls = {}, {}
    for fold in (False, True):
        monkeypatch.setattr(blocks, "_SC_FOLD", fold)
        counter = _CountConv(ops.lib)
        monkeypatch.setattr(ops, "lib", counter)
        with torch.no_grad():
            y = unet(x, 981).sample
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "lib", counter.raw)
        outs[fold], calls[fold] = y.float().clone(), counter.n
        if fold:
            folded_blocks = [m for m in unet.modules() if isinstance(m, blocks.ResnetBlock2D) and _plan_folds(m, 1)]
    # the halo-patch sites of batch 64: the three up-path blocks at 32^2, the first down block and the three up-path blocks at 16^2
    # (the 8^2 / 4^2 tiles take three taps per K step, the 2^2 level runs dense layers: two launches there)
    assert len(folded_blocks) == 7, len(folded_blocks)
    assert calls[False] - calls[True] == len(folded_blocks), (calls, len(folded_blocks))
    assert rel_rms(outs[True], outs[False].cpu()) <= 2e-2
