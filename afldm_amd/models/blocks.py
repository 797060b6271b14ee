"""diffusers-compatible building blocks of UNet2DModel, executing on libafldm_hip.so.

Constructor arguments, attribute names and state-dict keys follow diffusers 0.32.1 (the
package the reference builds on: reference afldm/af_modules/af_blocks.py:6-7,
afldm/pipelines/cross_frame_attn.py:3), so unmodified diffusers checkpoints load and the
reference's module surgery (af_api.py) applies as-is.

INTERNAL TENSOR CONVENTION: inside a UNet forward every activation is an NHWC ("channels
last") contiguous CUDA tensor [B, H, W, C] in the model dtype — the layout the MFMA implicit
GEMM, the attention kernel ([B, HW, C] is the same memory) and the alias-free kernels want.
`UNet2DModel.forward` converts from/to the public NCHW layout at its boundary.  A "virtual
concat" (the up-block skip torch.cat) is passed around as a tuple (x1, x2) and resolved inside
the kernels (two base pointers), never materialised.
"""
import math
import os
from typing import NamedTuple

import torch
import torch.nn as nn

from .. import aql, ops

# A ResnetBlock2D's 1x1 conv_shortcut runs inside its conv2 - extra centre-tap K steps of the halo-patch kernel over the block input,
# one bias b2 + b_sc - where afldm_conv2d_shortcut_ok allows it, instead of a launch of its own whose output conv2 re-reads as its
# residual.  AFLDM_NO_SHORTCUT_FOLD=1: the two launches (A/B).
_SC_FOLD = os.environ.get("AFLDM_NO_SHORTCUT_FOLD", "0") != "1"
# The same fold on the halo-patch tiles that take THREE filter taps per K step (the 8^2 / 4^2 levels - split-K slabs included -
# and every level at the small batches), a switch of its own so that the two are A/B-able independently (_SC_FOLD keeps meaning
# the one-tap tiles).  AFLDM_NO_SHORTCUT_FOLD3=1: the two launches there.
_SC_FOLD3 = os.environ.get("AFLDM_NO_SHORTCUT_FOLD3", "0") != "1"
# Which launches a ResnetBlock2D issues for an input is resolved once into a _ResnetPlan, cached per module in `_afldm_plan` under a
# key that holds the input's shape / dtype / device AND the current value of every switch the plan depends on (the two above,
# _CONST2, ops._C8, ops._DENSE2_MIN_B, AFLDM_NO_FUSED_ACT, AFLDM_NO_DENSE2X2): flipping a switch gives another plan, there is no cache to drop.
# Fixed, each after its measurement:
#  - at the 32^2 / 16^2 levels the activations WRITE 8-channel blocks and the convolutions behind them read them, conv1 writes NHWC:
#    4.754 ms/step against 4.804 (no blocks) / 4.785 (all three edges) / 4.827 (conv1 -> act2 only), profiles/r05/c8_layout_ab.txt;
#  - a conv_shortcut that stays a launch sits between the second activation and conv2 (`aql.independent`): the other positions
#    gained 0.006 - 0.018 ms under the AQL diagnostic library only, profiles/r05/aql_headers.txt;
#  - no merged activation -> convolution launches (ops.af_act_conv2d): 4.99 -> 5.01 / 5.09 ms/step, profiles/r05/actconv_ab.txt.


def _pair(x):
    return x if isinstance(x, tuple) else (x, None)


class PackedMixin:
    """Caches kernel-ready copies of parameters (OHWI weights in the activation dtype, fp32
    biases / affine params).  Invalidated by _apply (.to / .cuda / .half ...) and load_state_dict."""

    def _packed(self, key, build):
        cache = self.__dict__.setdefault("_afldm_cache", {})
        if key not in cache:
            cache[key] = build()
        return cache[key]

    def _invalidate(self):
        self.__dict__.pop("_afldm_cache", None)


def invalidate_packed(module: nn.Module):
    for m in module.modules():
        m.__dict__.pop("_afldm_cache", None)


def _weights_key(module: nn.Module):
    """What the packed copies are made from: every parameter's and buffer's storage, in-place version counter, dtype and device
    (tensors created under torch.inference_mode() have no version counter: -1)."""
    def ver(t):
        try:
            return t._version
        except RuntimeError:
            return -1
    return hash(tuple((t.data_ptr(), ver(t), t.dtype, str(t.device)) for t in (*module.parameters(), *module.buffers())))


def invalidate_stale_packed(module: nn.Module):
    """invalidate_packed, unless the packed copies were already dropped for the module's current weights.  Several cached graphs
    of one model (a ddim_inversion engine, a cross-frame sampler's engines) notice a weight change one after the other; a
    later one must not drop the copies that an earlier one has packed and captured since, or that graph replays freed memory.
    Returns True when it dropped them."""
    key = _weights_key(module)
    if module.__dict__.get("_afldm_packed_for") == key:
        return False
    invalidate_packed(module)
    module.__dict__["_afldm_packed_for"] = key
    return True


def packed_conv(mod, dtype):
    """(OHWI weight in `dtype`, fp32 bias) for an nn.Conv2d / nn.Linear, cached on the module."""
    cache = mod.__dict__.setdefault("_afldm_cache", {})
    key = ("w", dtype)
    if key not in cache:
        w = ops.pack_weight(mod.weight, dtype)
        b = None if mod.bias is None else mod.bias.detach().to(torch.float32).contiguous()
        cache[key] = (w, b)
    return cache[key]


def packed_qkv(attn, dtype, which):
    """Row-concatenated (to_q | to_k | to_v subset) OHWI weight + fp32 bias, cached on the module."""
    cache = attn.__dict__.setdefault("_afldm_cache", {})
    key = ("qkv", dtype, which)
    if key not in cache:
        mods = [getattr(attn, "to_" + n) for n in which]
        w = torch.cat([m.weight.detach().float() for m in mods], 0)
        b = torch.cat([m.bias.detach().float() for m in mods], 0).contiguous()
        cache[key] = (ops.pack_weight(w, dtype), b)
    return cache[key]


def packed_vo(attn, dtype):
    """The folded value-and-output projection of an attention block whose attention map is the identity (perturbed-attention
    guidance): W_vo = W_o W_v formed in fp64 and rounded ONCE to `dtype` (packed like a Linear weight), b_vo = W_o b_v + b_o
    formed in fp64 and kept in fp32.  One GEMM instead of to_v then to_out[0], and one rounding fewer than that chain.  Cached on
    the module and dropped with the other packed copies (invalidate_packed / invalidate_stale_packed)."""
    cache = attn.__dict__.setdefault("_afldm_cache", {})
    key = ("vo", dtype)
    if key not in cache:
        wo, wv = attn.to_out[0].weight.detach().double(), attn.to_v.weight.detach().double()
        b = attn.to_out[0].bias.detach().double()
        if attn.to_v.bias is not None:
            b = b + wo @ attn.to_v.bias.detach().double()
        cache[key] = (ops.pack_weight((wo @ wv).float(), dtype), b.float().contiguous())
    return cache[key]


def packed_norm(mod):
    cache = mod.__dict__.setdefault("_afldm_cache", {})
    if "gn" not in cache:
        cache["gn"] = (mod.weight.detach().to(torch.float32).contiguous(),
                       mod.bias.detach().to(torch.float32).contiguous())
    return cache["gn"]


def packed_conv_dense2x2(conv, dtype, C1, C2):
    """A 3x3 'same' convolution on a 2x2 plane is ONE dense layer over the flattened plane: output
    pixel p = (oh, ow) sees input pixel q = (ih, iw) through tap (ih - oh + 1, iw - ow + 1), which
    always lies inside the kernel.  W2[(p, n), (q, c)] = W[n, c, ih-oh+1, iw-ow+1], columns ordered
    like the NHWC flattening of the (virtually concatenated) input: [x1: q*C1 + c | x2: q*C2 + c].
    The implicit GEMM would spend 5 of its 9 taps on zero padding here (2.25x the flops)."""
    cache = conv.__dict__.setdefault("_afldm_cache", {})
    key = ("dense2x2", dtype, C1, C2)
    if key not in cache:
        W = conv.weight.detach().float()                       # [Cout, Cin, 3, 3]
        Cout = W.shape[0]
        assert W.shape[1] == C1 + C2 and tuple(W.shape[2:]) == (3, 3)
        parts = []
        for lo, hi in ((0, C1), (C1, C1 + C2)):
            if hi == lo:
                continue
            blk = torch.zeros(4, Cout, 4, hi - lo, dtype=torch.float32, device=W.device)
            for pidx in range(4):
                oh, ow = divmod(pidx, 2)
                for qidx in range(4):
                    ih, iw = divmod(qidx, 2)
                    blk[pidx, :, qidx, :] = W[:, lo:hi, ih - oh + 1, iw - ow + 1]
            parts.append(blk.reshape(4 * Cout, 4 * (hi - lo)))
        w2 = torch.cat(parts, 1).contiguous()
        b2 = None if conv.bias is None else conv.bias.detach().float().repeat(4).contiguous()
        cache[key] = (ops.pack_weight(w2, dtype), b2)
    return cache[key]


# The alias-free activation of a 2x2 plane is plane-constant (lpf(4) = [1,0,0,0]: reference ideal_lpf.py:17-21), so the 3x3 convolutions
# behind it are dense layers over Cin columns with tap-summed weights (packed_conv_dense2x2_const): a quarter of the 2x2 level's weight
# bytes (330 -> 83 MB per step).  AFLDM_NO_CONST2=1: the full flattened-plane form (A/B).
_CONST2 = os.environ.get("AFLDM_NO_CONST2", "0") != "1"


def packed_conv_dense2x2_const(conv, dtype):
    """A 3x3 'same' convolution of a PLANE-CONSTANT 2x2 input a[b, c] (the output of WarpedNonlinearity at N = 2): output pixel
    p = (oh, ow) sees every input pixel q through tap (ih - oh + 1, iw - ow + 1), and all four carry the same value, so
    y[b, (p, n)] = sum_c (sum_q W[n, c, tap(p, q)]) a[b, c]: the dense layer of packed_conv_dense2x2 with its four column blocks
    added up - Ws[(p, n), c] = W[n, c, 1-oh : 3-oh, 1-ow : 3-ow].sum().  Summed in fp64, rounded once to `dtype`."""
    cache = conv.__dict__.setdefault("_afldm_cache", {})
    key = ("dense2x2_const", dtype)
    if key not in cache:
        W = conv.weight.detach().double()                      # [Cout, Cin, 3, 3]
        assert tuple(W.shape[2:]) == (3, 3)
        blocks = [W[:, :, 1 - oh:3 - oh, 1 - ow:3 - ow].sum((2, 3)) for oh in (0, 1) for ow in (0, 1)]
        ws = torch.cat(blocks, 0).float().contiguous()         # [4 * Cout, Cin], row = pixel * Cout + n
        b2 = None if conv.bias is None else conv.bias.detach().float().repeat(4).contiguous()
        cache[key] = (ops.pack_weight(ws, dtype), b2)
    return cache[key]


def packed_conv_dense2x2_const_cm(conv, dtype):
    """packed_conv_dense2x2_const with its rows ordered channel-major (row = 4 n + pixel instead of pixel * Cout + n): a GroupNorm
    group of the output - cpg channels x 4 pixels - is then 4 cpg ADJACENT rows, what afldm_conv2x2_const_norm_act tiles over."""
    cache = conv.__dict__.setdefault("_afldm_cache", {})
    key = ("dense2x2_const_cm", dtype)
    if key not in cache:
        W = conv.weight.detach().double()
        Cout = W.shape[0]
        blocks = [W[:, :, 1 - oh:3 - oh, 1 - ow:3 - ow].sum((2, 3)) for oh in (0, 1) for ow in (0, 1)]      # [pixel][Cout, Cin]
        ws = torch.stack(blocks, 1).reshape(4 * Cout, -1).float().contiguous()                             # row = 4 n + pixel
        cache[key] = ops.pack_weight(ws, dtype)
    return cache[key]


def conv_forward(conv: nn.Conv2d, x, **kw):
    """F.conv2d(x, conv.weight, conv.bias, stride 1, 'same') on NHWC (or a virtual concat)."""
    x1, x2 = _pair(x)
    if (x1.ndim == 4 and x1.shape[1] == 2 and x1.shape[2] == 2 and tuple(conv.kernel_size) == (3, 3)
            and kw.get("out_mode", 0) == 0 and "out" not in kw and x1.shape[-1] % 8 == 0
            and (x2 is None or x2.shape[-1] % 8 == 0) and conv.out_channels % 8 == 0
            and not os.environ.get("AFLDM_NO_DENSE2X2")):
        B, C1, C2, Cout = x1.shape[0], x1.shape[-1], 0 if x2 is None else x2.shape[-1], conv.out_channels
        w2, b2 = packed_conv_dense2x2(conv, x1.dtype, C1, C2)
        kw = dict(kw)
        res = kw.pop("residual", None)
        if kw.get("temb") is not None:
            kw["temb_mod"] = Cout
        y = ops.conv2d(x1.reshape(B, 4 * C1), w2, b2, x2=None if x2 is None else x2.reshape(B, 4 * C2),
                       residual=None if res is None else res.reshape(B, 4 * Cout), **kw)
        out = y.view(B, 2, 2, Cout)
        st = getattr(y, "gn_partial", None)
        if st is not None:                                      # [B, S, 4*Cout, 2] -> per-pixel splits of Cout channels
            out.gn_partial = st.reshape(B, st.shape[1] * 4, Cout, 2)
        return out
    if (x2 is None and x1.ndim == 4 and x1.shape[-1] == 3 and tuple(conv.kernel_size) == (3, 3)
            and x1.dtype == torch.bfloat16 and conv.out_channels % 16 == 0 and (x1.shape[1] * x1.shape[2]) % 128 == 0):
        # RGB conv_in of the VAE encoder: a zero 4th channel puts it on the MFMA conv_in kernel
        # (k_conv_cin4_mfma) instead of the scalar small-Cin kernel (580 -> ~90 us at 8 x 256^2)
        cache = conv.__dict__.setdefault("_afldm_cache", {})
        key = ("w_cin4", x1.dtype)
        if key not in cache:
            w4 = torch.nn.functional.pad(conv.weight.detach().float(), (0, 0, 0, 0, 0, 1))      # [Cout, 4, 3, 3]
            cache[key] = (ops.pack_weight(w4, x1.dtype),
                          None if conv.bias is None else conv.bias.detach().to(torch.float32).contiguous())
        w, b = cache[key]
        return ops.conv2d(torch.nn.functional.pad(x1, (0, 1)), w, b, **kw)
    w, b = packed_conv(conv, x1.dtype)
    return ops.conv2d(x1, w, b, x2=x2, **kw)


def linear_forward(lin: nn.Linear, x, **kw):
    w, b = packed_conv(lin, x.dtype)
    return ops.conv2d(x, w, b, **kw)


# ----------------------------------------------------------------------------- embeddings
class Timesteps(nn.Module):
    def __init__(self, num_channels, flip_sin_to_cos, downscale_freq_shift):
        super().__init__()
        self.num_channels = num_channels
        self.flip_sin_to_cos = flip_sin_to_cos
        self.downscale_freq_shift = downscale_freq_shift

    def forward(self, timesteps, dtype=torch.float32):
        """timesteps: device float32 [rows] -> [rows, num_channels] in `dtype`."""
        return ops.timestep_embedding(timesteps, self.num_channels, self.flip_sin_to_cos,
                                      float(self.downscale_freq_shift), dtype)


class TimestepEmbedding(nn.Module):
    def __init__(self, in_channels, time_embed_dim, act_fn="silu"):
        super().__init__()
        assert act_fn == "silu"
        self.linear_1 = nn.Linear(in_channels, time_embed_dim)
        self.act = nn.SiLU()
        self.linear_2 = nn.Linear(time_embed_dim, time_embed_dim)

    def forward(self, sample):
        h = linear_forward(self.linear_1, sample)
        h = ops.silu(h)
        return linear_forward(self.linear_2, h)


# ----------------------------------------------------------------------------- resampling
class Downsample2D(nn.Module):
    """diffusers.models.downsampling.Downsample2D (conv variant, stride 2).  The vanilla
    stride-2 path is not on the alias-free hot path: only AliasFreeDownsample2D executes."""

    def __init__(self, channels, use_conv=False, out_channels=None, padding=1, name="conv", kernel_size=3,
                 norm_type=None, eps=None, elementwise_affine=None, bias=True):
        super().__init__()
        self.channels = channels
        self.out_channels = out_channels or channels
        self.use_conv = use_conv
        self.padding = padding
        self.name = name
        self.norm = None
        assert norm_type is None, "norm_type is not used by the FFHQ / AF-VAE configs"
        if use_conv:
            conv = nn.Conv2d(self.channels, self.out_channels, kernel_size=kernel_size, stride=2, padding=padding,
                             bias=bias)
        else:
            assert self.channels == self.out_channels
            conv = nn.AvgPool2d(kernel_size=2, stride=2)
        if name == "conv":
            self.Conv2d_0 = conv
            self.conv = conv
        elif name == "Conv2d_0":
            self.conv = conv
        else:
            self.conv = conv

    def forward(self, hidden_states, *args, **kwargs):
        raise NotImplementedError(
            "afldm_amd executes the alias-free model by default: call make_af_unet(unet) "
            "(afldm.af_modules.af_api) before running, or opt in to the vanilla resamplers with "
            "enable_vanilla_resampling(model) (same module); this Downsample2D has not been swapped")


class Upsample2D(nn.Module):
    """diffusers.models.upsampling.Upsample2D (nearest x2 + conv).  See Downsample2D."""

    def __init__(self, channels, use_conv=False, use_conv_transpose=False, out_channels=None, name="conv",
                 kernel_size=None, padding=1, norm_type=None, eps=None, elementwise_affine=None, bias=True,
                 interpolate=True):
        super().__init__()
        self.channels = channels
        self.out_channels = out_channels or channels
        self.use_conv = use_conv
        self.use_conv_transpose = use_conv_transpose
        self.name = name
        self.interpolate = interpolate
        self.norm = None
        assert norm_type is None and not use_conv_transpose
        conv = None
        if use_conv:
            if kernel_size is None:
                kernel_size = 3
            conv = nn.Conv2d(self.channels, self.out_channels, kernel_size=kernel_size, padding=padding, bias=bias)
        if name == "conv":
            self.conv = conv
        else:
            self.Conv2d_0 = conv

    def forward(self, hidden_states, output_size=None, *args, **kwargs):
        raise NotImplementedError(
            "afldm_amd executes the alias-free model by default: call make_af_unet(unet) first, or opt in to the "
            "vanilla resamplers with enable_vanilla_resampling(model) (afldm.af_modules.af_api); this Upsample2D "
            "has not been swapped")


def _adopt(new, old):
    """Hand every registered submodule (the conv, under each of its names) of `old` to `new`: parameters are shared."""
    for key, m in old._modules.items():
        new._modules[key] = m
    return new


class StridedDownsample2D(Downsample2D):
    """Downsample2D with use_conv on HIP: the stride-2 3x3 convolution (afldm_conv2d_s2).  Same constructor, attributes and
    state-dict keys as Downsample2D; af_api.enable_vanilla_resampling installs it.  padding=1 pads every side by one,
    padding=0 is diffusers' F.pad(x, (0, 1, 0, 1)) in front of an unpadded conv (the VAE encoder)."""

    @classmethod
    def from_vanilla(cls, d):
        conv = d.conv
        new = cls(d.channels, d.use_conv, out_channels=d.out_channels, padding=d.padding, name=d.name,
                  kernel_size=conv.kernel_size[0], bias=conv.bias is not None)
        return _adopt(new, d)

    def forward(self, hidden_states, *args, **kwargs):
        if not self.use_conv:
            raise NotImplementedError("afldm_amd: Downsample2D(use_conv=False) (AvgPool2d) has no HIP path")
        x = hidden_states
        assert x.ndim == 4 and x.shape[-1] == self.channels and not ops.is_c8(x)          # NHWC
        conv = self.conv
        if tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (2, 2) or self.padding not in (0, 1):
            raise NotImplementedError(f"afldm_amd: Downsample2D kernel {conv.kernel_size} / stride {conv.stride} / "
                                      f"padding {self.padding} has no HIP path (3x3, stride 2, padding 0 or 1)")
        w, b = packed_conv(conv, x.dtype)
        return ops.conv2d_s2(x, w, b, pad=(1, 1) if self.padding == 1 else (0, 1), want_stats=True)


class NearestUpsample2D(Upsample2D):
    """Upsample2D with use_conv on HIP: nearest x2 fused into the 3x3 convolution in phase-decomposed form
    (afldm_conv2d_up2, weights folded once per dtype by afldm_pack_weight_up2).  Same constructor, attributes and
    state-dict keys as Upsample2D; af_api.enable_vanilla_resampling installs it."""

    @classmethod
    def from_vanilla(cls, u):
        conv = u.conv if u.name == "conv" else u.Conv2d_0
        new = cls(u.channels, u.use_conv, u.use_conv_transpose, out_channels=u.out_channels, name=u.name,
                  kernel_size=None if conv is None else conv.kernel_size[0],
                  padding=1 if conv is None else conv.padding[0], bias=conv is not None and conv.bias is not None,
                  interpolate=u.interpolate)
        return _adopt(new, u)

    def forward(self, hidden_states, output_size=None, *args, **kwargs):
        x = hidden_states
        assert x.ndim == 4 and x.shape[-1] == self.channels and not ops.is_c8(x)          # NHWC
        if not self.use_conv:
            raise NotImplementedError("afldm_amd: Upsample2D(use_conv=False) has no HIP path")
        conv = self.conv if self.name == "conv" else self.Conv2d_0
        if tuple(conv.kernel_size) != (3, 3) or tuple(conv.padding) != (1, 1) or tuple(conv.stride) != (1, 1):
            raise NotImplementedError(f"afldm_amd: Upsample2D conv kernel {conv.kernel_size} / padding {conv.padding} "
                                      "has no HIP path (3x3, padding 1)")
        H, W = x.shape[1], x.shape[2]
        if not self.interpolate:
            return conv_forward(conv, x, want_stats=True)
        if output_size is not None and tuple(output_size) != (2 * H, 2 * W):
            raise ValueError(f"NearestUpsample2D: output_size {tuple(output_size)} is not 2x the input {(H, W)}")
        cache = conv.__dict__.setdefault("_afldm_cache", {})
        key = ("up2", x.dtype)
        if key not in cache:
            cache[key] = (ops.pack_weight_up2(conv.weight, x.dtype),
                          None if conv.bias is None else conv.bias.detach().to(torch.float32).contiguous())
        w, b = cache[key]
        return ops.conv2d_up2(x, w, b, want_stats=True)


def _bias_f32(conv):
    cache = conv.__dict__.setdefault("_afldm_cache", {})
    if "bias_f32" not in cache:
        cache["bias_f32"] = None if conv.bias is None else conv.bias.detach().to(torch.float32).contiguous()
    return cache["bias_f32"]


def _plane2_view(y, B, Cout):
    """[B, 4 * Cout] output of a flattened-plane dense layer as the NHWC tensor [B, 2, 2, Cout], statistics carried along."""
    out = y.view(B, 2, 2, Cout)
    st = getattr(y, "gn_partial", None)
    if st is not None:                                      # [B, S, 4*Cout, 2] -> per-pixel splits of Cout channels
        out.gn_partial = st.reshape(B, st.shape[1] * 4, Cout, 2)
    return out


_WARPED = None


def _warped_nonlinearity():
    global _WARPED
    if _WARPED is None:
        from ..af_modules.af_blocks import WarpedNonlinearity as _WARPED          # (lazy: af_blocks imports this module)
    return _WARPED


def _fused_af_silu(act):
    """True for the alias-free SiLU that the fused kernels compute (WarpedNonlinearity around nn.SiLU)."""
    return isinstance(act, _warped_nonlinearity()) and act.fused_silu


class _ResnetPlan(NamedTuple):
    """What ResnetBlock2D.forward issues for one kind of input (ResnetBlock2D._plan)."""
    const2: bool        # the route: the plane-constant 2x2 form (_forward_const2) instead of the general one
    dense2: bool        # ... whose conv1 + temb -> norm2 -> act2 is the ONE launch afldm_conv2x2_const_norm_act
    c8_1: bool          # act1 writes 8-channel blocks, conv1 reads them (and writes NHWC)
    c8_2: bool          # act2 writes 8-channel blocks, conv2 reads them
    fold: int           # conv2 takes the 1x1 shortcut as extra K steps: 0 no, 1 on a one-tap tile, 2 on a three-tap tile
    slabs1: bool        # conv1 -> norm2 -> act2 from conv1's split-K slabs, if its plan splits K (ops.conv2d_slabs says at run time)
    slabs2: bool        # conv2 -> next_gn likewise
    norm_out: bool      # else conv2's epilogue is offered next_gn


# ----------------------------------------------------------------------------- resnet
class ResnetBlock2D(nn.Module):
    """diffusers ResnetBlock2D (time_embedding_norm='default', no up/down, output_scale 1).

    forward(x, temb_proj): `temb_proj` is this block's slice [rows, out_channels] of the
    batched time_emb_proj GEMM computed once per step by UNet2DModel (rows = 1 broadcast or B),
    i.e. time_emb_proj(nonlinearity(emb)) of the reference forward."""

    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout=0.0, temb_channels=512,
                 groups=32, groups_out=None, pre_norm=True, eps=1e-6, non_linearity="swish",
                 time_embedding_norm="default", output_scale_factor=1.0, use_in_shortcut=None):
        super().__init__()
        assert time_embedding_norm == "default" and output_scale_factor == 1.0
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.output_scale_factor = output_scale_factor
        self.time_embedding_norm = time_embedding_norm
        groups_out = groups if groups_out is None else groups_out
        self.norm1 = nn.GroupNorm(num_groups=groups, num_channels=in_channels, eps=eps, affine=True)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.time_emb_proj = nn.Linear(temb_channels, out_channels) if temb_channels is not None else None
        self.norm2 = nn.GroupNorm(num_groups=groups_out, num_channels=out_channels, eps=eps, affine=True)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.nonlinearity = nn.SiLU()
        self.upsample = self.downsample = None
        self.use_in_shortcut = self.in_channels != out_channels if use_in_shortcut is None else use_in_shortcut
        self.conv_shortcut = None
        if self.use_in_shortcut:
            self.conv_shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0, bias=True)

    def _plan(self, x1, x2, temb_proj, temb_stride, next_gn):
        """The _ResnetPlan of this input under the switches as they stand now (cached in `_afldm_plan`; the probes behind a new
        plan run at the first call for a shape - an engine's warm-up step)."""
        af = _fused_af_silu(self.nonlinearity)
        key = (tuple(x1.shape), None if x2 is None else x2.shape[-1], x1.dtype, x1.device, temb_proj is not None, int(temb_stride),
               None if next_gn is None else (next_gn.num_groups, next_gn.num_channels), af,
               ops._C8, _SC_FOLD, _SC_FOLD3, _CONST2, ops._DENSE2_MIN_B,
               os.environ.get("AFLDM_NO_FUSED_ACT"), os.environ.get("AFLDM_NO_DENSE2X2"))
        plans = self.__dict__.setdefault("_afldm_plan", {})
        if key not in plans:
            plans[key] = self._make_plan(x1, x2, temb_proj, temb_stride, next_gn, af)
        return plans[key]

    def _make_plan(self, x1, x2, temb_proj, temb_stride, next_gn, af):
        """af: the nonlinearity is the fused alias-free SiLU."""
        B, N, C1, C2 = x1.shape[0], x1.shape[1], x1.shape[-1], 0 if x2 is None else x2.shape[-1]
        Cin, Cout, dt = C1 + C2, self.out_channels, x1.dtype
        fused = not os.environ.get("AFLDM_NO_FUSED_ACT")
        square = x1.ndim == 4 and x1.shape[1] == x1.shape[2]
        k3_1, k3_2 = tuple(self.conv1.kernel_size) == (3, 3), tuple(self.conv2.kernel_size) == (3, 3)
        # conv2's result straight into next_gn: afldm_af_act_slabs reads the residual as dense [B, N, N, Cout] - there is no res_ld,
        # so it must have Cout channels; that it is contiguous needs no check here (the shortcut's output is fresh, and a block input
        # that is not contiguous is refused by ops._dev in the first gn_stats)
        gn_ok = fused and next_gn is not None and Cout % next_gn.num_groups == 0 and next_gn.num_channels == Cout
        res_ok = self.conv_shortcut is not None or C1 == Cout
        if self._const2_form(x1, x2, af):
            dense2 = fused and ops.conv2x2_const_norm_act_ok(Cin, Cout, self.norm2.num_groups, dt, batch=B)
            return _ResnetPlan(True, dense2, False, False, 0, fused and not dense2, gn_ok and res_ok, False)
        c8 = ops._C8 and square and k3_1 and k3_2 and af and dt == torch.bfloat16 and N in (16, 32)
        can_fold = ((_SC_FOLD or _SC_FOLD3) and square and k3_2 and self.conv_shortcut is not None
                    and tuple(self.conv_shortcut.kernel_size) == (1, 1))
        c8_1 = c8_2 = False
        fold, sc = 0, None
        if c8 or can_fold:         # the probes carry what the real launches carry (ops.conv2d_c8_ok, ops.conv2d_shortcut_ok)
            h_in = torch.empty((B, N, N, Cout), dtype=dt, device=x1.device)          # stands for conv2's input
            w2, b2 = packed_conv(self.conv2, dt)
        if c8:
            w1, b1 = packed_conv(self.conv1, dt)
            a_in = torch.empty((B, N, N, Cin), dtype=dt, device=x1.device)
            c8_1 = ops.conv2d_c8_ok(a_in, w1, b1, temb=temb_proj, temb_stride=temb_stride)
            c8_2 = ops.conv2d_c8_ok(h_in, w2, b2, residual=h_in)
        if can_fold:
            sc = (x1, x2, packed_conv(self.conv_shortcut, dt)[0])
            if c8_2:
                h_in.c8 = True
            kind = ops.conv2d_shortcut_ok(h_in, w2, self._sc_bias(), sc)
            fold = kind if (kind == 1 and _SC_FOLD) or (kind == 2 and _SC_FOLD3) else 0
        slabs1 = square and self._slabs1_ok(N, Cin, af)
        slabs2 = square and N in (2, 4) and Cout % 8 == 0 and gn_ok and k3_2
        if fold:        # the slabs carry the shortcut only where the three-tap tile splits K (4x4 planes)
            slabs2 = slabs2 and N == 4 and ops.conv2d_shortcut_ok(h_in, w2, None, sc, slabs=True) == 2
        else:
            slabs2 = slabs2 and res_ok
        return _ResnetPlan(False, False, c8_1, c8_2, fold, slabs1, slabs2, next_gn is not None)

    def _const2_form(self, x1, x2, af):
        """The plane-constant 2x2 form applies: 2x2 planes under the fused alias-free SiLU, K of the two dense layers (Cin / Cout)
        whole K steps of the GEMM kernels (128 bytes of elements)."""
        C1, C2, Cout, kstep = x1.shape[-1], 0 if x2 is None else x2.shape[-1], self.out_channels, 128 // x1.element_size()
        return (_CONST2 and not os.environ.get("AFLDM_NO_DENSE2X2") and x1.ndim == 4 and x1.shape[1] == 2 and x1.shape[2] == 2 and af
                and tuple(self.conv1.kernel_size) == (3, 3) and tuple(self.conv2.kernel_size) == (3, 3)
                and C1 % 8 == 0 and C2 % 8 == 0 and Cout % 8 == 0 and Cout % self.norm2.num_groups == 0
                and (C1 + C2) % kstep == 0 and Cout % kstep == 0)

    def _slabs1_ok(self, N, Cin, af):
        """The static conditions of conv1 -> norm2 -> act2 from conv1's split-K slabs, on N x N planes of Cin channels."""
        Cout = self.out_channels
        return (af and not os.environ.get("AFLDM_NO_FUSED_ACT") and N in (2, 4) and tuple(self.conv1.kernel_size) == (3, 3)
                and Cin % 8 == 0 and Cout % 8 == 0 and Cout % self.norm2.num_groups == 0)

    def _sc_bias(self):
        """conv2.bias + conv_shortcut.bias, summed in fp64 and rounded once to fp32: the bias of conv2 with the shortcut folded in."""
        cache = self.__dict__.setdefault("_afldm_cache", {})
        if "sc_bias" not in cache:
            b = torch.zeros(self.out_channels, dtype=torch.float64, device=self.conv2.weight.device)
            for conv in (self.conv2, self.conv_shortcut):
                if conv.bias is not None:
                    b += conv.bias.detach().double()
            cache["sc_bias"] = b.float().contiguous()
        return cache["sc_bias"]

    def _norm_act(self, norm, x, out_c8=False, out_const=False):
        """norm -> self.nonlinearity fused: GroupNorm statistics, then either the fused
        GN + WarpedNonlinearity kernel (alias-free model) or GN + SiLU."""
        x1, x2 = _pair(x)
        gamma, beta = packed_norm(norm)
        stats = ops.gn_stats(x1, norm.num_groups, x2=x2)
        if _fused_af_silu(self.nonlinearity):
            return ops.af_act(x1, x2, stats, gamma, beta, norm.num_groups, norm.eps, out_c8=out_c8, out_const=out_const)
        if isinstance(self.nonlinearity, _warped_nonlinearity()):
            # a wrapped module other than SiLU: GroupNorm pass, then the module's own (unfused) alias-free form
            return self.nonlinearity(ops.gn_apply(x1, stats, gamma, beta, norm.num_groups, norm.eps, act=0, x2=x2))
        return ops.gn_apply(x1, stats, gamma, beta, norm.num_groups, norm.eps, act=1, x2=x2)

    def _slabs(self, conv, h, shortcut=None):
        """The split-K slabs of conv(h) (+ the folded shortcut) on a 2x2 / 4x4 plane, or None when the plan of this shape does
        not split K (the caller runs the ordinary sequence)."""
        B, N, _, Cin = h.shape
        if N == 2 and shortcut is None and not os.environ.get("AFLDM_NO_DENSE2X2"):
            w2, _ = packed_conv_dense2x2(conv, h.dtype, Cin, 0)          # one dense layer over the flattened plane
            return ops.conv2d_slabs(h.reshape(B, 4 * Cin), w2)
        return ops.conv2d_slabs(h, packed_conv(conv, h.dtype)[0], shortcut=shortcut)

    def _finish_slabs(self, got, bias, norm, B, N, dtype, temb=None, temb_stride=0, act=True, residual=None, raw=False):
        """A convolution's split-K slabs finished by the consumer of its output (afldm_af_act_slabs: no reduction launch, no
        stored intermediate): + bias (+ temb) (+ residual) -> GroupNorm `norm` -> act (True: the alias-free activation, 2: its
        plane-constant [B, C] form, False: none).  raw: the finished convolution output itself is stored too and returned, the
        normalised tensor attached as `.gn_applied = (tensor, norm module)` for AttnProcessor2_0."""
        slabs, nslab = got
        gamma, beta = packed_norm(norm)
        out = ops.af_act_slabs(slabs, nslab, bias, temb, temb_stride, gamma, beta, norm.num_groups, norm.eps, B, N, self.out_channels,
                               dtype, residual=residual, want_raw=raw, act=act)
        if not raw:
            return out
        hn, y = out
        y.gn_applied = (hn, norm)
        return y

    def _conv1_norm2_act_fused(self, h, temb_proj, temb_stride):
        """conv1 -> norm2 -> WarpedNonlinearity on the 2x2 / 4x4 planes when conv1 splits K: the activation kernel takes the
        convolution's fp32 slabs and finishes them itself.  Returns None when this shape / plan does not qualify (the caller runs
        the ordinary sequence)."""
        if (isinstance(h, tuple) or h.ndim != 4 or h.shape[1] != h.shape[2]
                or not self._slabs1_ok(h.shape[1], h.shape[-1], _fused_af_silu(self.nonlinearity))):
            return None
        return self._conv1_from_slabs(h, temb_proj, temb_stride)

    def _conv1_from_slabs(self, h, temb_proj, temb_stride):
        got = self._slabs(self.conv1, h)
        if got is None:
            return None
        return self._finish_slabs(got, _bias_f32(self.conv1), self.norm2, h.shape[0], h.shape[1], h.dtype, temb_proj, temb_stride)

    def _const2_ok(self, input_tensor):
        x1, x2 = _pair(input_tensor)
        return self._const2_form(x1, x2, _fused_af_silu(self.nonlinearity))

    def _forward_const2(self, plan, input_tensor, temb_proj, temb_stride, next_gn):
        """The block on 2x2 planes: both alias-free activations are plane-constant there, so they are stored once per plane
        ([B, C]) and conv1 / conv2 run as dense layers over Cin / Cout columns with tap-summed weights
        (packed_conv_dense2x2_const) - same function, a quarter of the weight bytes and of the GEMM's K."""
        x1, x2 = _pair(input_tensor)
        B, dt, Cout = x1.shape[0], x1.dtype, self.out_channels
        a = self._norm_act(self.norm1, input_tensor, out_const=True)                 # [B, Cin]
        if plan.dense2:
            # conv1 + temb -> norm2 -> activation in ONE launch: a workgroup owns a whole GroupNorm group of the dense layer's columns
            g2, be2 = packed_norm(self.norm2)
            h = ops.conv2x2_const_norm_act(a, packed_conv_dense2x2_const_cm(self.conv1, dt), _bias_f32(self.conv1), temb_proj,
                                           temb_stride, g2, be2, self.norm2.num_groups, self.norm2.eps)
        else:
            w1, b1 = packed_conv_dense2x2_const(self.conv1, dt)
            got = ops.conv2d_slabs(a, w1) if plan.slabs1 else None
            if got is not None:
                h = self._finish_slabs(got, _bias_f32(self.conv1), self.norm2, B, 2, dt, temb_proj, temb_stride, act=2)
            else:
                kw = dict(temb=temb_proj, temb_stride=temb_stride, temb_mod=Cout) if temb_proj is not None else {}
                y = ops.conv2d(a, w1, b1, want_stats=True, **kw)                         # [B, 4 * Cout]
                h = self._norm_act(self.norm2, _plane2_view(y, B, Cout), out_const=True)
        res = conv_forward(self.conv_shortcut, input_tensor) if self.conv_shortcut is not None else x1
        assert self.conv_shortcut is not None or x2 is None
        w2, b2 = packed_conv_dense2x2_const(self.conv2, dt)
        got = ops.conv2d_slabs(h, w2) if plan.slabs2 else None
        if got is not None:                    # conv2 + residual straight into the attention block's GroupNorm
            return self._finish_slabs(got, _bias_f32(self.conv2), next_gn, B, 2, dt, residual=res, act=False, raw=True)
        y = ops.conv2d(h, w2, b2, residual=res.reshape(B, 4 * Cout), want_stats=True)
        return _plane2_view(y, B, Cout)

    def forward(self, input_tensor, temb_proj=None, temb_stride=0, next_gn=None):
        """next_gn: the GroupNorm module of an attention block that consumes this block's output next (the block loops
        pass it): lets conv2 hand its result over already normalised where that saves launches."""
        x1, x2 = _pair(input_tensor)
        plan = self._plan(x1, x2, temb_proj, temb_stride, next_gn)
        if plan.const2:
            return self._forward_const2(plan, input_tensor, temb_proj, temb_stride, next_gn)
        # act1
        h = self._norm_act(self.norm1, input_tensor, out_c8=plan.c8_1)
        # conv1 (+ norm2 / act2): from conv1's split-K slabs in one launch, or conv1 (its epilogue emits norm2's statistics) -> act2
        fused = self._conv1_from_slabs(h, temb_proj, temb_stride) if plan.slabs1 else None
        if fused is None:
            h = conv_forward(self.conv1, h, temb=temb_proj, temb_stride=temb_stride, want_stats=True)
            h = self._norm_act(self.norm2, h, out_c8=plan.c8_2)
        else:
            h = fused
        # shortcut: extra K steps of conv2, a launch of its own (independent of everything above: afldm_amd/aql.py), or the input
        sc = res = None
        if plan.fold:
            sc = (x1, x2, packed_conv(self.conv_shortcut, h.dtype)[0])
        elif self.conv_shortcut is not None:
            with aql.independent("shortcut"):
                res = conv_forward(self.conv_shortcut, input_tensor)
        else:
            assert x2 is None
            res = x1
        # conv2 (+ the next norm): from conv2's split-K slabs (4x4 / 2x2 planes), from its own epilogue (8x8: one tile = one
        # whole sample), or left to the attention block
        if plan.slabs2:
            got = self._slabs(self.conv2, h, shortcut=sc)
            if got is not None:
                return self._finish_slabs(got, self._sc_bias() if plan.fold else _bias_f32(self.conv2), next_gn, h.shape[0],
                                          h.shape[1], h.dtype, residual=res, act=False, raw=True)
        kw = {}
        if plan.norm_out:
            gamma, beta = packed_norm(next_gn)
            kw["norm_out"] = (gamma, beta, next_gn.num_groups, next_gn.eps)
        if plan.fold:
            out = ops.conv2d(h, packed_conv(self.conv2, h.dtype)[0], self._sc_bias(), want_stats=True, shortcut=sc, **kw)
        else:
            out = conv_forward(self.conv2, h, residual=res, want_stats=True, **kw)
        hn = getattr(out, "norm_applied", None)
        if hn is not None:
            out.gn_applied = (hn, next_gn)
        return out


def _next_gn(attn):
    """The GroupNorm an attention block will apply to its input, when its processor is the plain self-attention one
    (a cross-frame processor normalises / stores on its own terms: no hand-over)."""
    if attn is None or attn.group_norm is None or type(attn.processor) is not AttnProcessor2_0:
        return None
    return attn.group_norm


# ----------------------------------------------------------------------------- attention
class AttnProcessor2_0:
    """diffusers AttnProcessor2_0 for the self-attention 'attn block' configuration
    (residual_connection=True, rescale_output_factor=1), on NHWC tensors.

    encoder_hidden_states, when given, is the already group-normed K/V source [Bk, HW, C]
    (the protocol CrossFrameAttnProcessor uses, reference cross_frame_attn.py:125)."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, kv=None, kv_sink=None,
                 kv1=None, alpha=None, qk_sink=None, src=None):
        """kv / kv_sink (CrossFrameAttnProcessor with cache_kv): `kv_sink(k, vt)` receives this call's projected keys
        [B, T, C] (a view) and channel-major values [B, C, T] - the self-attention then runs on the three-launch path, where
        they exist in memory; `kv = (k, vt)` runs the attention against such a stored pair (Bk divides B) instead of projecting
        an encoder_hidden_states map: K / V of the stored pass are the same numbers whichever pass projects them.
        kv1 + alpha (the interpolating processor): a second stored pair, and the output is
        to_out((1 - alpha) attn(q, kv) + alpha attn(q, kv1)) + residual with alpha [B] fp32 on the device - one
        afldm_attention_interp launch and one to_out GEMM (to_out is affine and the residual is common to both terms).
        src + alpha (the banked processor): `kv = (k, vt)` is a bank of S stored sources and src [B, 2] int32 on the device names
        every sample's two (ops.attention_bank: one launch, then the one to_out + residual as on the interp path).
        qk_sink (SAGAttnProcessor): `qk_sink(q, k)` receives this call's projected queries and keys [B, T, C] (views of the
        q | k buffer) in front of the attention launch; like kv_sink it sends the block to the three-launch path."""
        assert attention_mask is None
        assert kv1 is None or (kv is not None and alpha is not None)
        assert src is None or (kv is not None and alpha is not None and kv1 is None)
        B, H, W, C = hidden_states.shape
        gamma, beta = packed_norm(attn.group_norm)
        gn = attn.group_norm
        pre = getattr(hidden_states, "gn_applied", None)
        plain = kv is None and kv_sink is None and qk_sink is None
        assert qk_sink is None or (kv is None and encoder_hidden_states is None), "qk_sink observes plain self-attention"
        assert kv is None or encoder_hidden_states is None
        if (plain and pre is None and encoder_hidden_states is None and C // attn.heads <= 32
                and ops.attn_block_fused_ok(hidden_states.view(B, H * W, C), attn.heads, gn.num_groups)):
            # 32^2 / 16^2 levels, bf16: GroupNorm-apply + q | k | v projection + attention in ONE launch (csrc/attnf.hip)
            stats = ops.gn_stats(hidden_states, gn.num_groups)
            w, b = packed_qkv(attn, hidden_states.dtype, ("q", "k", "v"))
            if ops.attn_block_fused_out_ok(hidden_states.view(B, H * W, C), attn.heads, gn.num_groups):
                # ... and to_out + the residual connection in the same launch (32^2 level)
                wo, bo = packed_conv(attn.to_out[0], hidden_states.dtype)
                y = ops.attn_block_fused_out(hidden_states.view(B, H * W, C), stats, gamma, beta, gn.num_groups, gn.eps, w, b,
                                             attn.heads, attn.scale, wo, bo)
                return ops.carry_stats(y.view(B, H, W, C), y)
            o = ops.attn_block_fused(hidden_states.view(B, H * W, C), stats, gamma, beta, gn.num_groups, gn.eps, w, b,
                                     attn.heads, attn.scale)
            return linear_forward(attn.to_out[0], o.view(B, H, W, C), residual=hidden_states, want_stats=True)
        if pre is not None and pre[1] is gn:
            hn = pre[0]                                   # the producing resnet block already applied this GroupNorm
        else:
            stats = ops.gn_stats(hidden_states, gn.num_groups)
            hn = ops.gn_apply(hidden_states, stats, gamma, beta, gn.num_groups, gn.eps, act=0)
        tokens = hn.view(B, H * W, C)
        if C // attn.heads > 32:
            # large head_dim (the VAE mid block: one head of 512): GEMM - row softmax - GEMM per sample
            assert plain, "kv / kv_sink cover head_dim <= 32 (the UNet's attention blocks)"
            src = tokens if encoder_hidden_states is None else encoder_hidden_states
            q = linear_forward(attn.to_q, tokens)
            k = linear_forward(attn.to_k, src)
            vt = linear_forward(attn.to_v, src, out_mode=1)
            o = ops.attention_dense(q, k, vt, attn.scale)
            return linear_forward(attn.to_out[0], o.view(B, H, W, C), residual=hidden_states, want_stats=True)
        if plain and encoder_hidden_states is None and ops.attn_small_fused_ok(tokens, attn.heads):
            # 8^2 / 4^2 levels, bf16: projection + attention in ONE launch on the normalised tokens (csrc/attns.hip)
            w, b = packed_qkv(attn, tokens.dtype, ("q", "k", "v"))
            o = ops.attn_small_fused(tokens, w, b, attn.heads, attn.scale)
            return linear_forward(attn.to_out[0], o.view(B, H, W, C), residual=hidden_states, want_stats=True)
        if kv is not None:
            q = linear_forward(attn.to_q, tokens)
            k, vt = kv
        elif encoder_hidden_states is None:
            # fused Q|K|V projection: one GEMM reads the normed tokens once; Q and K land token-major
            # side by side, V channel-major (the attention kernel's V^T operand)
            w, b = packed_qkv(attn, tokens.dtype, ("q", "k", "v"))
            qk, vt = ops.linear_split(tokens, w, b, 2 * C)
            q, k = qk[:, :, :C], qk[:, :, C:]
            if kv_sink is not None:
                kv_sink(k, vt)
            if qk_sink is not None:
                qk_sink(q, k)
        else:
            q = linear_forward(attn.to_q, tokens)
            w, b = packed_qkv(attn, tokens.dtype, ("k", "v"))
            k, vt = ops.linear_split(encoder_hidden_states, w, b, C)
        if src is not None:
            o = ops.attention_bank(q, k, vt, src, alpha, attn.heads, scale=attn.scale)
        elif kv1 is not None:
            o = ops.attention_interp(q, k, vt, kv1[0], kv1[1], alpha, attn.heads, scale=attn.scale)
        else:
            o = ops.attention(q, k, vt, attn.heads, scale=attn.scale)
        return linear_forward(attn.to_out[0], o.view(B, H, W, C), residual=hidden_states, want_stats=True)


class PAGAttnProcessor(AttnProcessor2_0):
    """Perturbed-attention guidance (Ahn et al. 2024; diffusers PAGIdentitySelfAttnProcessor2_0) on a batch of 2 B: rows 0 .. B-1
    run the plain block, rows B .. 2B-1 the block with its attention map replaced by the identity,
    y = x + to_out(to_v(GN(x))), as one launch on the folded weight (ops.attn_identity_block, packed_vo).  The two halves are
    joined by a concatenating copy into one [2B, H, W, C] tensor: the plain half is whatever launch list AttnProcessor2_0 chooses
    for B rows and allocates its own output.  The result carries no GroupNorm partial sums (the next block makes its own pass),
    and because _next_gn tests the processor type exactly, the resnet in front hands no pre-normed tensor to such a site."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, **kwargs):
        assert encoder_hidden_states is None and attention_mask is None and not kwargs, "PAG perturbs plain self-attention"
        B2, H, W, C = hidden_states.shape
        if B2 % 2:
            raise ValueError(f"PAGAttnProcessor: a batch of {B2} rows (want the plain rows followed by as many perturbed ones)")
        B = B2 // 2
        gn = attn.group_norm
        gamma, beta = packed_norm(gn)
        out = torch.empty_like(hidden_states)
        out[:B].copy_(super().__call__(attn, hidden_states[:B]))
        xp = hidden_states[B:]
        stats = ops.gn_stats(xp, gn.num_groups)
        w, b = packed_vo(attn, hidden_states.dtype)
        ops.attn_identity_block(xp, stats, gamma, beta, gn.num_groups, gn.eps, w, b, out=out[B:])
        return out


class SAGAttnProcessor(AttnProcessor2_0):
    """Self-attention guidance (Hong et al., ICCV 2023; diffusers StableDiffusionSAGPipeline's attention hook) at ONE site: the
    plain block, run on the three-launch path where q and k exist in memory (the kv_sink route), plus one
    ops.attn_key_mass call on them: the attention mass each key receives, fp32 [B, T], written into `mass` - a buffer the engine
    owns (a captured graph writes the same address at every replay), or one made per call and kept in `self.mass` when none is
    given.  The block's output is AttnProcessor2_0's with a no-op kv_sink, bit for bit: the extra launches only read q and k.
    Because _next_gn tests the processor type exactly, the resnet in front hands no pre-normed tensor to such a site."""

    def __init__(self, mass=None):
        self.mass = mass
        self._given = mass is not None

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, **kwargs):
        assert encoder_hidden_states is None and attention_mask is None and not kwargs, "SAG observes plain self-attention"
        if hidden_states.shape[-1] // attn.heads > 32:
            raise NotImplementedError("SAGAttnProcessor: head_dim > 32 has no key-mass kernel")

        def sink(q, k):
            self.mass = ops.attn_key_mass(q, k, attn.heads, scale=attn.scale, out=self.mass if self._given else None)

        return super().__call__(attn, hidden_states, qk_sink=sink)


class Attention(nn.Module):
    """diffusers.models.attention_processor.Attention restricted to what UNet2DModel's attention
    blocks use (self-attention, group_norm, bias, residual connection)."""

    def __init__(self, query_dim, heads=8, dim_head=64, rescale_output_factor=1.0, eps=1e-5, norm_num_groups=None,
                 residual_connection=False, bias=False, upcast_softmax=False, _from_deprecated_attn_block=False,
                 processor=None, **unused):
        super().__init__()
        assert rescale_output_factor == 1.0
        self.inner_dim = dim_head * heads
        self.query_dim = query_dim
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.rescale_output_factor = rescale_output_factor
        self.residual_connection = residual_connection
        self.norm_cross = None
        self.spatial_norm = None
        self.group_norm = (nn.GroupNorm(num_channels=query_dim, num_groups=norm_num_groups, eps=eps, affine=True)
                           if norm_num_groups is not None else None)
        self.to_q = nn.Linear(query_dim, self.inner_dim, bias=bias)
        self.to_k = nn.Linear(query_dim, self.inner_dim, bias=bias)
        self.to_v = nn.Linear(query_dim, self.inner_dim, bias=bias)
        self.to_out = nn.ModuleList([nn.Linear(self.inner_dim, query_dim, bias=True), nn.Dropout(0.0)])
        self.processor = processor if processor is not None else AttnProcessor2_0()

    def set_processor(self, processor):
        self.processor = processor

    def get_processor(self, return_deprecated_lora=False):
        return self.processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **kwargs):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states,
                              attention_mask=attention_mask, **kwargs)


# ----------------------------------------------------------------------------- UNet blocks
class _BlockBase(nn.Module):
    def _resnets(self, in_cs, out_c, temb_channels, eps, groups, dropout):
        return nn.ModuleList([
            ResnetBlock2D(in_channels=c, out_channels=out_c, temb_channels=temb_channels, eps=eps, groups=groups,
                          dropout=dropout) for c in in_cs])

    def _attns(self, n, c, head_dim, eps, groups):
        return nn.ModuleList([
            Attention(c, heads=c // head_dim, dim_head=head_dim, eps=eps, norm_num_groups=groups,
                      residual_connection=True, bias=True, upcast_softmax=True, _from_deprecated_attn_block=True)
            for _ in range(n)])


class DownBlock2D(_BlockBase):
    has_attention = False

    def __init__(self, in_channels, out_channels, temb_channels, num_layers=1, resnet_eps=1e-6, resnet_groups=32,
                 dropout=0.0, add_downsample=True, downsample_padding=1, attention_head_dim=1):
        super().__init__()
        self.resnets = self._resnets([in_channels if i == 0 else out_channels for i in range(num_layers)],
                                     out_channels, temb_channels, resnet_eps, resnet_groups, dropout)
        if self.has_attention:
            self.attentions = self._attns(num_layers, out_channels, attention_head_dim, resnet_eps, resnet_groups)
        self.downsamplers = (nn.ModuleList([Downsample2D(out_channels, use_conv=True, out_channels=out_channels,
                                                         padding=downsample_padding, name="op")])
                             if add_downsample else None)

    def forward(self, hidden_states, temb_slices):
        outs = ()
        for i, resnet in enumerate(self.resnets):
            hidden_states = resnet(hidden_states, *temb_slices[i], next_gn=_next_gn(self.attentions[i]) if self.has_attention else None)
            if self.has_attention:
                hidden_states = self.attentions[i](hidden_states)
            outs += (hidden_states,)
        if self.downsamplers is not None:
            for d in self.downsamplers:
                hidden_states = d(hidden_states)
            outs += (hidden_states,)
        return hidden_states, outs


class AttnDownBlock2D(DownBlock2D):
    has_attention = True


class UNetMidBlock2D(_BlockBase):
    def __init__(self, in_channels, temb_channels, dropout=0.0, num_layers=1, resnet_eps=1e-6, resnet_groups=32,
                 attn_groups=None, add_attention=True, attention_head_dim=1):
        super().__init__()
        self.add_attention = add_attention
        if attn_groups is None:
            attn_groups = resnet_groups
        self.resnets = self._resnets([in_channels] * (num_layers + 1), in_channels, temb_channels, resnet_eps,
                                     resnet_groups, dropout)
        self.attentions = (self._attns(num_layers, in_channels, attention_head_dim, resnet_eps, attn_groups)
                           if add_attention else nn.ModuleList([None] * num_layers))

    def forward(self, hidden_states, temb_slices=None):
        if temb_slices is None:                       # VAE: no time embedding
            temb_slices = [(None, 0)] * len(self.resnets)
        hidden_states = self.resnets[0](hidden_states, *temb_slices[0], next_gn=_next_gn(self.attentions[0]) if len(self.attentions) else None)
        for i, (attn, resnet) in enumerate(zip(self.attentions, self.resnets[1:])):
            if attn is not None:
                hidden_states = attn(hidden_states)
            hidden_states = resnet(hidden_states, *temb_slices[i + 1])
        return hidden_states


class UpBlock2D(_BlockBase):
    has_attention = False

    def __init__(self, in_channels, prev_output_channel, out_channels, temb_channels, num_layers=1, resnet_eps=1e-6,
                 resnet_groups=32, dropout=0.0, add_upsample=True, attention_head_dim=1):
        super().__init__()
        in_cs = []
        for i in range(num_layers):
            res_skip = in_channels if (i == num_layers - 1) else out_channels
            rin = prev_output_channel if i == 0 else out_channels
            in_cs.append(rin + res_skip)
        self.resnets = self._resnets(in_cs, out_channels, temb_channels, resnet_eps, resnet_groups, dropout)
        if self.has_attention:
            self.attentions = self._attns(num_layers, out_channels, attention_head_dim, resnet_eps, resnet_groups)
        self.upsamplers = (nn.ModuleList([Upsample2D(out_channels, use_conv=True, out_channels=out_channels)])
                           if add_upsample else None)

    def forward(self, hidden_states, res_hidden_states_tuple, temb_slices):
        for i, resnet in enumerate(self.resnets):
            res = res_hidden_states_tuple[-1]
            res_hidden_states_tuple = res_hidden_states_tuple[:-1]
            hidden_states = resnet((hidden_states, res), *temb_slices[i],      # virtual torch.cat([h, res], 1)
                                   next_gn=_next_gn(self.attentions[i]) if self.has_attention else None)
            if self.has_attention:
                hidden_states = self.attentions[i](hidden_states)
        if self.upsamplers is not None:
            for u in self.upsamplers:
                hidden_states = u(hidden_states)
        return hidden_states


class AttnUpBlock2D(UpBlock2D):
    has_attention = True


DOWN_BLOCKS = {"DownBlock2D": DownBlock2D, "AttnDownBlock2D": AttnDownBlock2D}
UP_BLOCKS = {"UpBlock2D": UpBlock2D, "AttnUpBlock2D": AttnUpBlock2D}
