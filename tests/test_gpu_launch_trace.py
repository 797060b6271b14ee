"""GPU test: the sequence of library launches that ResnetBlock2D (and the UNet around it) issues, with the arguments that select a
kernel, against tests/golden/resnet_launch_trace.json - recorded from the commit before ResnetBlock2D resolved its routes into one
cached plan (`python tests/test_gpu_launch_trace.py --record`) and copied here unchanged.  A refactor of the block's Python must
leave every sequence as it is; the switch cases flip one switch per case WITHOUT dropping any cache, and the default case after
them must equal the first one (the plan key holds the switches).

Every case is traced on its second forward: the first one packs weights and filters (launches of their own, once per module)."""
import contextlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet_launch_trace.json")
QUERIES = ("_ok", "_workspace", "_variant", "_stats_splits", "_supported")
CONV_INTS = ("B", "H", "W", "C1", "C2", "Cout", "KS", "x_layout", "y_layout")
CONV_INTS_2 = ("defer_reduce", "out_mode", "temb_stride")
CONV_PTRS = ("residual", "stats_out", "y_norm", "temb", "workspace")

# one switch per case: (module, attribute, value) or ("env", variable, value)
FLIPS = {
    "sc_fold_off": ("blocks", "_SC_FOLD", False),
    "sc_fold3_off": ("blocks", "_SC_FOLD3", False),
    "c8_off": ("ops", "_C8", False),
    "const2_off": ("blocks", "_CONST2", False),
    "no_fused_act": ("env", "AFLDM_NO_FUSED_ACT", "1"),
    "no_dense2x2": ("env", "AFLDM_NO_DENSE2X2", "1"),
}
# single alias-free blocks (bf16, batch 64, no next_gn): plane, input channels C1 | C2, Cout
AF_BLOCKS = [(8, 768, 384, 384), (4, 768, 768, 768), (2, 768, 0, 768)]


class _Trace:
    """ops.lib with every launching call noted in order: the calls whose last argument is the current stream (the rule of
    ops._end); the queries are left out (their number changes with the caches)."""

    def __init__(self, raw):
        self.raw, self.calls = raw, []

    def __getattr__(self, name):
        f = getattr(self.raw, name)
        if name.endswith(QUERIES):
            return f

        def traced(*a):
            if a and a[-1] == stream_ptr():
                self.calls.append(_entry(name, a))
            return f(*a)
        return traced


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _entry(name, a):
    if name == "afldm_conv2d":
        c = a[0]._obj                                   # the ConvArgs behind the byref
        return ([name] + [int(getattr(c, k)) for k in CONV_INTS] + [int(c.sc_C1 + c.sc_C2)] + [int(getattr(c, k)) for k in CONV_INTS_2]
                + [int(bool(getattr(c, k))) for k in CONV_PTRS])
    if name == "afldm_af_act_slabs":                    # (slabs, nslab, bias, temb, temb_stride, residual, raw, gamma, beta, G, eps, act, ...)
        return [name, int(a[11]), int(bool(a[5])), int(bool(a[6]))]
    return [name]


@contextlib.contextmanager
def _flipped(flip):
    from afldm_amd import ops
    from afldm_amd.models import blocks
    where, name, value = flip
    if where == "env":
        old = os.environ.get(name)
        os.environ[name] = value
    else:
        mod = {"blocks": blocks, "ops": ops}[where]
        old = getattr(mod, name)
        setattr(mod, name, value)
    try:
        yield
    finally:
        if where != "env":
            setattr(mod, name, old)
        elif old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _drop_plans(model):
    """--record only: the commit the fixture is recorded from keeps per-module plan caches that do not know the switches."""
    for m in model.modules():
        for k in [k for k in m.__dict__ if k.startswith("_afldm_") and k not in ("_afldm_cache", "_afldm_packed_for")]:
            del m.__dict__[k]


def _trace(model, run, record=False):
    """The launches of the second `run()` (see the module docstring), on a stream of its own so that the stream argument is
    no small integer a query could carry."""
    from afldm_amd import ops
    if record:
        _drop_plans(model)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), torch.no_grad():
        run()
        proxy = _Trace(ops.lib)
        ops.lib = proxy
        try:
            run()
        finally:
            ops.lib = proxy.raw
    stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    assert proxy.calls, "nothing was launched"
    return proxy.calls


def _unet(dtype):
    from test_gpu_r02 import build_unet
    unet, cfg, _ = build_unet("ffhq", dtype)
    return unet, cfg


def _unet_run(unet, cfg, B, dtype):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, cfg["in_channels"], cfg["sample_size"], cfg["sample_size"], generator=g).cuda().to(dtype)
    return lambda: unet(x, 981).sample


def _af_block_run(N, C1, C2, Cout, per_sample_temb):
    from afldm_amd.af_modules.af_blocks import WarpedNonlinearity
    from afldm_amd.models import blocks
    B, dtype = 64, torch.bfloat16
    torch.manual_seed(5)
    blk = blocks.ResnetBlock2D(in_channels=C1 + C2, out_channels=Cout, temb_channels=64, groups=32, eps=1e-5)
    blk.nonlinearity = WarpedNonlinearity(blk.nonlinearity)
    blk = blk.cuda().to(dtype)
    g = torch.Generator().manual_seed(N + C1)
    x1 = torch.randn(B, N, N, C1, generator=g).cuda().to(dtype)
    inp = (x1, torch.randn(B, N, N, C2, generator=g).cuda().to(dtype)) if C2 else x1
    temb = torch.randn(B if per_sample_temb else 1, Cout, generator=g).cuda().to(dtype)
    if per_sample_temb:
        return blk, lambda: blk(inp, temb, Cout)
    return blk, lambda: blk(inp, temb.view(-1), 0)


def _plain_block_run(dtype):
    """The VAE's block: plain SiLU, no time embedding."""
    from afldm_amd.models import blocks
    torch.manual_seed(5)
    blk = blocks.ResnetBlock2D(in_channels=64, out_channels=128, temb_channels=None, groups=32, eps=1e-6).cuda().to(dtype)
    x = torch.randn(2, 16, 16, 64, generator=torch.Generator().manual_seed(16)).cuda().to(dtype)
    return blk, lambda: blk(x)


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def _cases(record=False):
    """(case name, trace) of every case, in the order they must run in."""
    unet, cfg = _unet(torch.bfloat16)
    for B in (64, 8, 1):
        yield f"unet_bf16_b{B}", _trace(unet, _unet_run(unet, cfg, B, torch.bfloat16), record)
    run = _unet_run(unet, cfg, 64, torch.bfloat16)
    for name, flip in FLIPS.items():
        with _flipped(flip):
            yield f"unet_bf16_b64_{name}", _trace(unet, run, record)
    yield "unet_bf16_b64_again", _trace(unet, run, record)
    del unet, run
    unet, cfg = _unet(torch.float32)
    yield "unet_fp32_b8", _trace(unet, _unet_run(unet, cfg, 8, torch.float32), record)
    del unet
    for N, C1, C2, Cout in AF_BLOCKS:
        for per_sample in (False, True):
            blk, run = _af_block_run(N, C1, C2, Cout, per_sample)
            yield f"af_block_n{N}_temb_{'rows' if per_sample else 'one'}", _trace(blk, run, record)
    for dtype in (torch.float32, torch.bfloat16):
        blk, run = _plain_block_run(dtype)
        yield f"plain_block_{_name(dtype)}", _trace(blk, run, record)


def _golden():
    with open(FIXTURE) as f:
        return json.load(f)


def _same(name, got, want):
    n = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    if n < max(len(got), len(want)):
        print(f"[launch trace] {name}: {len(got)} launches, recorded {len(want)}; first difference at index {n}:")
        print("   now     ", got[n] if n < len(got) else None)
        print("   recorded", want[n] if n < len(want) else None)
    assert got == want, (name, n)


@pytest.fixture(scope="module")
def unet_bf16():
    return _unet(torch.bfloat16)


@pytest.mark.parametrize("B", [64, 8, 1])
def test_unet_launch_sequence_bf16(unet_bf16, B):
    unet, cfg = unet_bf16
    _same(f"unet_bf16_b{B}", _trace(unet, _unet_run(unet, cfg, B, torch.bfloat16)), _golden()[f"unet_bf16_b{B}"])


def test_unet_launch_sequence_fp32():
    unet, cfg = _unet(torch.float32)
    _same("unet_fp32_b8", _trace(unet, _unet_run(unet, cfg, 8, torch.float32)), _golden()["unet_fp32_b8"])


def test_unet_launch_sequence_under_each_switch(unet_bf16):
    """One switch flipped per case on ONE model, no cache dropped in between; the default sequence is back afterwards."""
    unet, cfg = unet_bf16
    want = _golden()
    run = _unet_run(unet, cfg, 64, torch.bfloat16)
    first = _trace(unet, run)
    _same("unet_bf16_b64", first, want["unet_bf16_b64"])
    for name, flip in FLIPS.items():
        with _flipped(flip):
            got = _trace(unet, run)
        _same(f"unet_bf16_b64_{name}", got, want[f"unet_bf16_b64_{name}"])
        assert got != first, f"{name}: the switch changes the launches"
    again = _trace(unet, run)
    _same("unet_bf16_b64_again", again, want["unet_bf16_b64_again"])
    assert again == first


@pytest.mark.parametrize("per_sample_temb", [False, True])
@pytest.mark.parametrize("N,C1,C2,Cout", AF_BLOCKS)
def test_af_block_launch_sequence(N, C1, C2, Cout, per_sample_temb):
    name = f"af_block_n{N}_temb_{'rows' if per_sample_temb else 'one'}"
    blk, run = _af_block_run(N, C1, C2, Cout, per_sample_temb)
    _same(name, _trace(blk, run), _golden()[name])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plain_block_launch_sequence(dtype):
    blk, run = _plain_block_run(dtype)
    _same(f"plain_block_{_name(dtype)}", _trace(blk, run), _golden()[f"plain_block_{_name(dtype)}"])


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"], "usage: test_gpu_launch_trace.py --record [output.json]"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    traces = dict(_cases(record=True))
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in traces.items()) + "\n}\n")
    print("recorded", {k: len(v) for k, v in traces.items()}, "->", out)
