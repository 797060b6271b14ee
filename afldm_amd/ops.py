"""Tensor-level wrappers over the C ABI (include/afldm_hip.h).  PyTorch here is only the owner
of device memory and streams; every op below is one or two HIP kernel launches from
libafldm_hip.so on torch's current stream.  All activations are NHWC ([B, H, W, C]) or
token-major ([B, T, C]) contiguous CUDA tensors in fp32 or bf16.  CPU tensors raise."""
import collections
import contextlib
import ctypes
import math
import os

import torch

from . import _exp, _lib
from ._lib import AfActArgs, ConvArgs, DTYPE_CODE, SepArgs, check, stream_ptr

_FILTER_CACHE = {}
_PROFILE = None


class _RecordingLib:
    """libafldm_hip.so's entry points.  Outside a Profiler this is a plain pass-through; inside one every call is also
    noted as (function, arguments) so that the launches between _begin() and _end() can be re-issued later on the
    same buffers: bench.py captures each kernel family's launches of one step into a HIP graph and times the replay
    (kernel time without host gaps).  The stream is the last argument of every launching entry point; a replay
    substitutes the stream that is current then."""

    def __init__(self, raw):
        self._raw = raw
        self._wrapped = {}

    def __getattr__(self, name):
        w = self._wrapped.get(name)
        if w is None:
            f = getattr(self._raw, name)

            def w(*a, _f=f):
                if _PROFILE is not None:
                    _PROFILE.pending.append((_f, a))
                return _f(*a)
            self._wrapped[name] = w
        return w


lib = _RecordingLib(_lib.lib)


def ptr(t):
    """Device address of a tensor (None -> NULL).  Under a Profiler the tensor is also kept alive, so that a recorded
    launch can be replayed on buffers that still hold the step's real activations."""
    if t is None:
        return None
    if _PROFILE is not None:
        _PROFILE.live.append(t)
    return t.data_ptr()


class Profiler:
    """Per-op HIP-event timing on the launch stream (bench.py's roofline leg).  Records, per
    wrapper call, the kernel family, its ALGORITHMIC flops / bytes and two events around it."""

    def __init__(self):
        self.records = []
        self.pending = []        # (function, args) of the library calls since the last _begin()
        self.live = []           # tensors whose addresses went into recorded calls

    def __enter__(self):
        global _PROFILE
        _PROFILE = self
        return self

    def __exit__(self, *a):
        global _PROFILE
        _PROFILE = None

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for kind, flops, nbytes, e0, e1, _ in self.records:
            d = agg.setdefault(kind, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return agg


def _begin():
    if _PROFILE is None:
        return None
    _PROFILE.pending = []
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _replay_of(calls):
    """Re-issue recorded launches on the current stream (their last argument is the stream)."""
    def replay():
        st = stream_ptr()
        for f, a in calls:
            check(f(*a[:-1], st), "replay")
    return replay


def _end(tok, kind, flops=0.0, nbytes=0.0, replay=None):
    """replay: a callable that re-issues exactly this launch on the same buffers (bench.py replays a family's launches
    back to back from a captured graph to time the kernels without the host's launch gaps)."""
    if tok is None:
        return
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    if replay is None:
        st = stream_ptr()
        calls = [(f, a) for f, a in _PROFILE.pending if a and a[-1] == st]       # launches only (queries take no stream)
        if calls:
            replay = _replay_of(calls)
    _PROFILE.pending = []
    _PROFILE.records.append((kind, float(flops), float(nbytes), tok, e, replay))


def _dev(t, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"afldm_amd: {name} must live on an MI355X (cuda) device; there is no CPU path")
    if not t.is_contiguous():
        raise RuntimeError(f"afldm_amd: {name} must be contiguous")
    return t


def _code(t):
    try:
        return DTYPE_CODE[t.dtype]
    except KeyError:
        raise RuntimeError(f"afldm_amd: dtype {t.dtype} unsupported (fp32 / bf16 only)")


def filter_matrices(N, device):
    """(U [2N,N], D [N,2N]) device fp32 matrices for a plane of size N (cached per device)."""
    key = ("act", N, str(device))
    if key not in _FILTER_CACHE:
        U = _lib.filter_matrix(0, N, 2).to(device)
        D = _lib.filter_matrix(1, 2 * N).to(device)
        _FILTER_CACHE[key] = (U, D)
    return _FILTER_CACHE[key]


def packed_filters(N, dtype, device):
    """Device LDS image of (U, D) for the MFMA alias-free activation (N = 16, 32), cached."""
    if N < 4:
        return None
    key = ("packed", N, dtype, str(device))
    if key not in _FILTER_CACHE:
        U, D = filter_matrices(N, device)
        nbytes = lib.afldm_af_pack_bytes(N, DTYPE_CODE[dtype])
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        check(lib.afldm_af_pack(ptr(U), ptr(D), N, DTYPE_CODE[dtype], ptr(buf), stream_ptr()), "af_pack")
        _FILTER_CACHE[key] = buf
    return _FILTER_CACHE[key]


def down_matrix(N, device):
    """D [N/2, N] for AliasFreeDownsample2D on an N x N plane."""
    key = ("down", N, str(device))
    if key not in _FILTER_CACHE:
        _FILTER_CACHE[key] = _lib.filter_matrix(1, N).to(device)
    return _FILTER_CACHE[key]


def up_matrix(N, up, device):
    key = ("up", N, up, str(device))
    if key not in _FILTER_CACHE:
        _FILTER_CACHE[key] = _lib.filter_matrix(0, N, up).to(device)
    return _FILTER_CACHE[key]


# ----------------------------------------------------------------------------- layout
def to_nhwc(x, dtype=torch.float32, out=None):
    """NCHW fp32 -> NHWC dtype."""
    _dev(x, "x")
    assert x.dtype == torch.float32 and x.ndim == 4
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty((B, H, W, C), dtype=dtype, device=x.device)
    check(lib.afldm_nchw_to_nhwc(ptr(x), ptr(out), B, C, H, W, _code(out), stream_ptr()), "nchw_to_nhwc")
    return out


def to_nchw(x, out=None):
    """NHWC dtype -> NCHW fp32."""
    _dev(x, "x")
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    check(lib.afldm_nhwc_to_nchw(ptr(x), ptr(out), B, C, H, W, _code(x), stream_ptr()), "nhwc_to_nchw")
    return out


def pack_weight(w, dtype):
    """OIHW (or [O, I]) fp32 parameter -> OHWI dtype."""
    _dev(w, "weight")
    w = w.detach().to(torch.float32).contiguous()
    if w.ndim == 2:
        O, I = w.shape
        KH = KW = 1
    else:
        O, I, KH, KW = w.shape
    out = torch.empty((O, KH, KW, I), dtype=dtype, device=w.device)
    check(lib.afldm_pack_weight(ptr(w), ptr(out), O, I, KH, KW, _code(out), stream_ptr()), "pack_weight")
    return out


# ----------------------------------------------------------------------------- small ops
def timestep_embedding(t, dim, flip_sin_to_cos=True, freq_shift=0.0, dtype=torch.float32, out=None):
    _dev(t, "t")
    assert t.dtype == torch.float32 and t.ndim == 1
    rows = t.shape[0]
    if out is None:
        out = torch.empty((rows, dim), dtype=dtype, device=t.device)
    check(lib.afldm_timestep_embedding(ptr(t), ptr(out), rows, dim, int(flip_sin_to_cos), float(freq_shift),
                                       _code(out), stream_ptr()), "timestep_embedding")
    return out


def silu(x, out=None):
    _dev(x, "x")
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_silu(ptr(x), ptr(out), x.numel(), _code(x), stream_ptr()), "silu")
    return out


def _cat_args(x1, x2):
    _dev(x1, "x1")
    C1 = x1.shape[-1]
    if x2 is None:
        return C1, None, 0
    _dev(x2, "x2")
    assert x2.shape[:-1] == x1.shape[:-1] and x2.dtype == x1.dtype
    return C1, x2, x2.shape[-1]


_MAX_SPLITS = 32       # row splits of GroupNorm partial sums a consumer should have to walk


class GNStats:
    """Per-channel GroupNorm partial sums of a tensor or of a virtual concat x1|x2:
    st1 [B, S1, C1, 2], st2 [B, S2, C2, 2] fp32 (sum, sum of squares per pixel split).  Producers:
    gn_stats (stand-alone pass) and conv2d(..., want_stats=True) (GEMM epilogue, attached to the
    output tensor as `.gn_partial`).  Consumers finish mean / rstd themselves."""
    __slots__ = ("st1", "st2")

    def __init__(self, st1, st2=None):
        self.st1, self.st2 = st1, st2

    @property
    def S1(self):
        return self.st1.shape[1]

    @property
    def S2(self):
        return 0 if self.st2 is None else self.st2.shape[1]


def _tensor_stats(x, out=None):
    """Per-channel partial sums of ONE NHWC tensor: the ones its producing conv attached, else a pass."""
    st = getattr(x, "gn_partial", None)
    if st is not None and out is None:
        return st
    assert not getattr(x, "c8", False), "a tensor in 8-channel blocks carries its producer's statistics (no stand-alone pass)"
    _dev(x, "x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    S = lib.afldm_gn_stats_splits(HW)
    if out is None:
        out = torch.empty((B, S, C, 2), dtype=torch.float32, device=x.device)
    tok = _begin()
    check(lib.afldm_gn_stats(ptr(x), C, ptr(out), B, HW, _code(x), stream_ptr()), "gn_stats")
    _end(tok, "gn_stats", 0, B * HW * C * x.element_size())
    if st is None:
        x.gn_partial = out      # a skip connection is normalised twice (down block, then up block): one pass
    return out


def gn_stats(x1, G=None, x2=None, out=None):
    """GroupNorm statistics (GNStats) of the virtual concat x1|x2.  `G` is accepted for source
    compatibility and ignored: the partial sums are per channel, any grouping is formed by the
    consumer.  `out` (single tensor only) forces a stand-alone pass into that buffer."""
    C1, x2, C2 = _cat_args(x1, x2)
    return GNStats(_tensor_stats(x1, out), None if x2 is None else _tensor_stats(x2))


def carry_stats(dst, src):
    """Views / reshapes create new tensor objects: hand the attached statistics over."""
    st = getattr(src, "gn_partial", None)
    if st is not None:
        dst.gn_partial = st
    return dst


def gn_mean_rstd(stats, G, n, eps):
    """(mean, rstd) [B, G] from GNStats - host-side helper for tests / debugging only."""
    parts = [stats.st1.double().sum(1)] + ([] if stats.st2 is None else [stats.st2.double().sum(1)])
    s = torch.cat(parts, 1)                                     # [B, C, 2]
    B, C, _ = s.shape
    s = s.view(B, G, C // G, 2).sum(2)
    mean = s[..., 0] / n
    var = (s[..., 1] / n - mean * mean).clamp_min(0)
    return mean.float(), (1.0 / torch.sqrt(var + eps)).float()


def _stats_ptrs(stats):
    if stats is None:
        return None, 0, None, 0
    return ptr(stats.st1), stats.S1, ptr(stats.st2), stats.S2


def gn_apply(x1, stats, gamma, beta, G, eps, act=0, x2=None, out=None):
    C1, x2, C2 = _cat_args(x1, x2)
    B = x1.shape[0]
    HW = x1.numel() // (B * C1)
    if out is None:
        out = torch.empty(tuple(x1.shape[:-1]) + (C1 + C2,), dtype=x1.dtype, device=x1.device)
    p1, S1, p2, S2 = _stats_ptrs(stats)
    tok = _begin()
    check(lib.afldm_gn_apply(ptr(x1), C1, ptr(x2), C2, p1, S1, p2, S2, ptr(gamma), ptr(beta), ptr(out), B, HW, G,
                             float(eps), int(act), _code(x1), stream_ptr()), "gn_apply")
    _end(tok, "gn_apply", 0, 2 * B * HW * (C1 + C2) * x1.element_size())
    return out


# ----------------------------------------------------------------------------- alias-free ops
# AFLDM_NO_C8=1: every tensor NHWC (A/B).  Default: inside a ResnetBlock2D of the 32^2 / 16^2 levels the tensors between the
# alias-free activations and the 3x3 convolutions travel in 8-channel blocks [B][C/8][N][N][8] (`.c8 = True` on the tensor
# object; same shape, same values): an activation item is a contiguous run then (profiles/r05/c8_layout_ab.txt).
_C8 = os.environ.get("AFLDM_NO_C8", "0") != "1"


def is_c8(x):
    return bool(getattr(x, "c8", False))


def af_act(x1, x2=None, stats=None, gamma=None, beta=None, G=0, eps=0.0, out=None, out_c8=False, out_const=False):
    """[GroupNorm-apply ->] WarpedNonlinearity(SiLU) on an NHWC tensor (virtual concat x1|x2).  out_c8: the output in
    8-channel blocks (tagged `.c8`); an input tagged `.c8` is read in that layout (N = 16 / 32, bf16).
    out_const (N = 2 only): the result of a 2 x 2 plane is plane-constant (lpf(4) = [1,0,0,0], ideal_lpf.py:17-21) - return
    it once per plane as [B, C] tagged `.const2` (afldm_af_act_const2)."""
    C1, x2, C2 = _cat_args(x1, x2)
    B, N, N2, _ = x1.shape
    assert N == N2, "the reference's ideal filters assume square planes (ideal_lpf.py:80)"
    if out_const:
        assert N == 2 and out is None and not is_c8(x1)
        out = torch.empty((B, C1 + C2), dtype=x1.dtype, device=x1.device)
        U, D = filter_matrices(2, x1.device)
        p1, S1, p2, S2 = _stats_ptrs(stats)
        tok = _begin()
        check(lib.afldm_af_act_const2(ptr(x1), C1, ptr(x2), C2, p1, S1, p2, S2, ptr(gamma), ptr(beta), int(G), float(eps), ptr(U),
                                      ptr(D), ptr(out), B, _code(x1), stream_ptr()), "af_act_const2")
        _end(tok, "af_act_N2", 24.0 * 8 * B * (C1 + C2), B * 5 * (C1 + C2) * x1.element_size())
        out.const2 = True
        return out
    if out is None:
        out = torch.empty((B, N, N, C1 + C2), dtype=x1.dtype, device=x1.device)
    if out_c8 or is_c8(x1):
        assert N in (16, 32) and x1.dtype == torch.bfloat16 and (x2 is None or not is_c8(x1)) and not is_c8(x2)
        U, D = filter_matrices(N, x1.device)
        packed = packed_filters(N, x1.dtype, x1.device)
        p1, S1, p2, S2 = _stats_ptrs(stats)
        tok = _begin()
        check(lib.afldm_af_act_c8(ptr(x1), C1, ptr(x2), C2, p1, S1, p2, S2, ptr(gamma), ptr(beta), int(G), float(eps), ptr(U),
                                  ptr(D), ptr(packed), ptr(out), B, N, _code(x1), 1 if is_c8(x1) else 0, 1 if out_c8 else 0,
                                  stream_ptr()), "af_act_c8")
        _end(tok, f"af_act_N{N}", 24.0 * N ** 3 * B * (C1 + C2), 2 * B * N * N * (C1 + C2) * x1.element_size())
        if out_c8:
            out.c8 = True
        return out
    if N > 32:
        if x2 is not None:
            raise RuntimeError("afldm_amd: the large-plane activation path (N > 32) does not take a virtual concat")
        if x1.dtype == torch.float32 and N > 64:
            # fp32 128^2 planes: the matrices do not fit LDS -> generic (VALU) separable products:
            # GN-apply, U x U^T, SiLU, D z D^T as four elementary launches (exact-parity mode only)
            xn = x1 if stats is None else gn_apply(x1, stats, gamma, beta, G, eps, act=0)
            U, D = filter_matrices(N, x1.device)
            return af_resample(silu(af_resample(xn, U)), D, out=out)
        return _af_act_large(x1, stats, gamma, beta, G, eps, out)
    U, D = filter_matrices(N, x1.device)
    packed = packed_filters(N, x1.dtype, x1.device)
    p1, S1, p2, S2 = _stats_ptrs(stats)
    tok = _begin()
    check(lib.afldm_af_act(ptr(x1), C1, ptr(x2), C2, p1, S1, p2, S2, ptr(gamma), ptr(beta), int(G), float(eps), ptr(U),
                           ptr(D), ptr(packed), ptr(out), B, N, _code(x1), stream_ptr()), "af_act")
    # dense separable form: 24 N^3 flop per plane; one read + one write of the tensor
    _end(tok, f"af_act_N{N}", 24.0 * N ** 3 * B * (C1 + C2), 2 * B * N * N * (C1 + C2) * x1.element_size())
    return out


AF_KERNELS = tuple(_lib.ABI.names("AFLDM_AF_ROUTE_"))           # ("plane", "kron", ...): the header's names, by value
RESAMPLE_KINDS = tuple(_lib.ABI.names("AFLDM_RESAMPLE_ROUTE_"))
AfRoute = collections.namedtuple("AfRoute", "kernel ch grid items_per_wg")
ResampleRoute = collections.namedtuple("ResampleRoute", "kind split")
_AF_TUNE_FIELDS = _lib.ABI.names("AFLDM_AF_TUNE_")               # {"ch": 1, "small_n": 2, ...}
_AF_TUNE_RESET = _AF_TUNE_FIELDS.pop("reset")


def af_act_route(dtype, N, C1, C2, B, cus=0, has_packed=None, has_UD=True):
    """The kernel af_act runs for such a call (afldm_af_act_route: the plan the launch itself follows).  cus = 0 asks the
    device; any other value plans for that many compute units and needs no GPU.  has_packed: as af_act passes it (N >= 4)."""
    out = (ctypes.c_int * 4)()
    has_packed = N >= 4 if has_packed is None else has_packed
    check(_lib.lib.afldm_af_act_route(DTYPE_CODE[dtype], N, C1, C2, B, cus, int(has_packed), int(has_UD), out), "af_act_route")
    return AfRoute(AF_KERNELS[out[0]], out[1], out[2], out[3])


def af_resample_route(N, C, R):
    """The route of af_up2 / af_lpf_down2 / af_resample inside afldm_af_resample (not the MFMA plane kernel that af_up2 /
    af_lpf_down2 pick themselves at 16 -> 32 / 32 -> 16)."""
    out = (ctypes.c_int * 2)()
    check(_lib.lib.afldm_af_resample_route(N, C, R, out), "af_resample_route")
    return ResampleRoute(RESAMPLE_KINDS[out[0]], out[1])


@contextlib.contextmanager
def af_tune(**fields):
    """Set fields of the activation / resampling planners (afldm_af_tune: ch, small_n, p8, stagger, no_resample_small,
    resample_split, max_grid) for the block; on exit every field is back at its environment default."""
    unknown = set(fields) - set(_AF_TUNE_FIELDS)
    if unknown:
        raise TypeError(f"af_tune: unknown field(s) {sorted(unknown)}")
    try:
        for name, value in fields.items():
            check(_lib.lib.afldm_af_tune(_AF_TUNE_FIELDS[name], int(value)), "af_tune")
        yield
    finally:
        check(_lib.lib.afldm_af_tune(_AF_TUNE_RESET, 0), "af_tune")


def _resample_plane(x, M, R, out, want_stats):
    """One-kernel MFMA resample (afldm_af_resample_plane) for the UNet's 16 -> 32 / 32 -> 16 sites."""
    B, N, _, C = x.shape
    st = torch.empty((B, 1, C, 2), dtype=torch.float32, device=x.device) if want_stats else None
    tok = _begin()
    check(lib.afldm_af_resample_plane(ptr(x), ptr(M), ptr(out), ptr(st), B, N, C, R, _code(x), stream_ptr()),
          "af_resample_plane")
    _end(tok, "af_resample_plane", 4.0 * (N * N * R + N * R * R) * B * C / 2, B * (N * N + R * R) * C * x.element_size())
    if st is not None:
        out.gn_partial = st
    return out


_PLANE_RESAMPLE = os.environ.get("AFLDM_NO_RESAMPLE_PLANE", "0") != "1"


def af_up2(x, out=None, workspace=None):
    _dev(x, "x")
    B, N, N2, C = x.shape
    assert N == N2
    U = up_matrix(N, 2, x.device)
    if out is None:
        out = torch.empty((B, 2 * N, 2 * N, C), dtype=x.dtype, device=x.device)
    if N >= 32 and C % 16 == 0 and (x.dtype == torch.bfloat16 or N <= 64):
        return _resample_large(x, U, 2 * N, out)
    if N == 16 and C % 16 == 0 and _PLANE_RESAMPLE:
        return _resample_plane(x, U, 32, out, False)
    if workspace is None:
        workspace = torch.empty(B * 2 * N * N * C, dtype=torch.float32, device=x.device)
    assert workspace.numel() >= B * 2 * N * N * C
    tok = _begin()
    check(lib.afldm_af_up2(ptr(x), ptr(U), ptr(out), ptr(workspace), B, N, C, _code(x), stream_ptr()), "af_up2")
    _end(tok, "af_up2", 12.0 * N ** 3 * B * C, 5 * B * N * N * C * x.element_size())
    return out


def af_lpf_down2(x, out=None, workspace=None, want_stats=False):
    _dev(x, "x")
    B, N, N2, C = x.shape
    assert N == N2
    D = down_matrix(N, x.device)
    if out is None:
        out = torch.empty((B, N // 2, N // 2, C), dtype=x.dtype, device=x.device)
    if N >= 64 and C % 16 == 0 and (x.dtype == torch.bfloat16 or N <= 128):
        return _resample_large(x, D, N // 2, out)
    if N == 32 and C % 16 == 0 and _PLANE_RESAMPLE:
        return _resample_plane(x, D, 16, out, want_stats)
    if workspace is None:
        workspace = torch.empty(B * (N // 2) * N * C, dtype=torch.float32, device=x.device)
    assert workspace.numel() >= B * (N // 2) * N * C
    st = None
    if want_stats and C % 4 == 0 and N <= 32 and N & (N - 1) == 0:
        st = torch.empty((B, N // 2, C, 2), dtype=torch.float32, device=x.device)    # one split per output row
    tok = _begin()
    check(lib.afldm_af_lpf_down2(ptr(x), ptr(D), ptr(out), ptr(workspace), ptr(st), B, N, C, _code(x), stream_ptr()),
          "af_lpf_down2")
    _end(tok, "af_lpf_down2", 1.5 * N ** 3 * B * C, 1.25 * B * N * N * C * x.element_size())
    if st is not None:
        out.gn_partial = st
    return out


# ----------------------------------------------------------------------------- large planes (AF-VAE)
def sep_pass(x, y, M, K, R, outer_count, inner_count, in_outer_stride, in_k_stride, out_outer_stride, out_k_stride,
             M2=None, R2=0, gn_table=None, C=0, outer_per_sample=1, act=0, up_identity=False):
    """One separable pass (afldm_sep_pass): y[line][r] = act(M xn[line]) or M2 silu(M xn[line]).
    up_identity: M is the x2 upsampler U, whose even rows are the identity (afldm_sep_args.up_identity)."""
    a = SepArgs()
    a.x, a.y, a.M, a.M2, a.gn_table = ptr(x), ptr(y), ptr(M), ptr(M2), ptr(gn_table)
    a.outer_count, a.inner_count = int(outer_count), int(inner_count)
    a.in_outer_stride, a.in_k_stride = int(in_outer_stride), int(in_k_stride)
    a.out_outer_stride, a.out_k_stride = int(out_outer_stride), int(out_k_stride)
    a.K, a.R, a.R2, a.C, a.outer_per_sample, a.act = int(K), int(R), int(R2), int(C), int(outer_per_sample), int(act)
    a.dtype = _code(x)
    a.up_identity = int(up_identity)       # True / 1: where it pays; 2: every size that has the form (tests)
    tok = _begin()
    check(lib.afldm_sep_pass(ctypes.byref(a), stream_ptr()), "sep_pass")
    lines = outer_count * inner_count
    _end(tok, "sep_pass", 2.0 * lines * K * R + (2.0 * lines * R * R2 if R2 else 0.0),
         lines * (K + (R2 if R2 else R)) * x.element_size())
    return y


def gn_table(stats, gamma, beta, B, C, G, HW, eps):
    """[B, C, 2] (scale, shift) table from GroupNorm partial sums (for the large-plane passes)."""
    out = torch.empty((B, C, 2), dtype=torch.float32, device=stats.st1.device)
    check(lib.afldm_gn_table(ptr(stats.st1), stats.S1, ptr(gamma), ptr(beta), ptr(out), B, C, G, HW, float(eps),
                             stream_ptr()), "gn_table")
    return out


_UP_IDENTITY = os.environ.get("AFLDM_NO_UP_IDENTITY", "0") != "1"


def _af_act_large(x, stats, gamma, beta, G, eps, out):
    """WarpedNonlinearity on planes too large for LDS (N >= 64): up-H, (up-W, SiLU, down-W) chained,
    down-H — three MFMA passes through HBM with intermediates in the activation dtype."""
    B, N, _, C = x.shape
    U, D = filter_matrices(N, x.device)
    table = gn_table(stats, gamma, beta, B, C, G, N * N, eps) if stats is not None else None
    t1 = torch.empty((B, 2 * N, N, C), dtype=x.dtype, device=x.device)
    sep_pass(x, t1, U, N, 2 * N, B, N * C, N * N * C, N * C, 2 * N * N * C, N * C,
             gn_table=table, C=C, outer_per_sample=1)
    v = torch.empty((B, 2 * N, N, C), dtype=x.dtype, device=x.device)
    sep_pass(t1, v, U, N, 2 * N, B * 2 * N, C, N * C, C, N * C, C, M2=D, R2=N, up_identity=_UP_IDENTITY)
    del t1
    sep_pass(v, out, D, 2 * N, N, B, N * C, 2 * N * N * C, N * C, N * N * C, N * C)
    return out


def _resample_large(x, M, R, out):
    """y = M x M^T per plane via two MFMA passes (planes N >= 32 of the AF-VAE)."""
    B, N, _, C = x.shape
    tmp = torch.empty((B, R, N, C), dtype=x.dtype, device=x.device)
    sep_pass(x, tmp, M, N, R, B, N * C, N * N * C, N * C, R * N * C, N * C)
    sep_pass(tmp, out, M, N, R, B * R, C, N * C, C, R * C, C)
    return out


def softmax_rows(x, scale=1.0, out=None):
    _dev(x, "x")
    cols = x.shape[-1]
    rows = x.numel() // cols
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_softmax_rows(ptr(x), ptr(out), rows, cols, float(scale), _code(x), stream_ptr()), "softmax_rows")
    return out


_BATCHED_DENSE_ATTN = os.environ.get("AFLDM_NO_BATCHED_DENSE_ATTN", "0") != "1"


def attention_dense(q, k, vt, scale):
    """Single-head attention with a large head_dim (the VAE mid block: d = 512, T = 1024) as two
    per-sample GEMMs around a row softmax.  q, k: [B, T, C] contiguous; vt: [B, C, T]."""
    B, T, C = q.shape
    Tk = k.shape[1]
    if k.shape[0] != B or tuple(k.shape) != (B, Tk, C) or tuple(vt.shape) != (B, C, Tk):
        raise RuntimeError(f"afldm_amd: attention_dense needs k [B, Tk, C] and vt [B, C, Tk] with q's batch; got q "
                           f"{tuple(q.shape)}, k {tuple(k.shape)}, vt {tuple(vt.shape)} (repeat shared K / V over the batch)")
    _dev(q, "q"), _dev(k, "k"), _dev(vt, "vt")
    out = torch.empty_like(q)
    if (_BATCHED_DENSE_ATTN and q.dtype == torch.bfloat16 and Tk == T and T % 128 == 0 and C % 64 == 0
            and B * T * max(T, C) * 2 < (1 << 31)):
        # the whole batch in three launches: sample b's K_b / V_b^T are the "weights" of its rows (afldm_conv_args.w_batch_stride)
        try:
            s = conv2d(q.view(B, T, 1, C), k[0].view(T, 1, 1, C), w_batch_stride=T * C)      # [B, T, 1, T] scores
        except RuntimeError as e:
            if "w_batch_stride" not in str(e):
                raise
            s = None       # the plan for this shape splits K / has a tile that straddles samples: per-sample launches below
        if s is not None:
            p = softmax_rows(s.view(B * T, T), scale)
            try:
                conv2d(p.view(B, T, 1, T), vt[0].view(C, 1, 1, T), w_batch_stride=C * T, out=out.view(B, T, 1, C))
                return out
            except RuntimeError as e:
                if "w_batch_stride" not in str(e):
                    raise
    for b in range(B):
        s = conv2d(q[b].view(1, T, 1, C), k[b].view(Tk, 1, 1, C))               # [1, T, 1, Tk] scores
        p = softmax_rows(s.view(T, Tk), scale)
        conv2d(p.view(1, T, 1, Tk), vt[b].view(C, 1, 1, Tk), out=out[b].view(1, T, 1, C))
    return out


def lpf_matrix(N, device):
    key = ("lpf", N, str(device))
    if key not in _FILTER_CACHE:
        _FILTER_CACHE[key] = _lib.filter_matrix(2, N).to(device)
    return _FILTER_CACHE[key]


def af_resample(x, M, out=None, workspace=None):
    """y = M x M^T per plane: [B,N,N,C] -> [B,R,R,C] with M [R,N] device fp32."""
    _dev(x, "x")
    B, N, N2, C = x.shape
    assert N == N2 and M.shape[1] == N
    R = M.shape[0]
    if out is None:
        out = torch.empty((B, R, R, C), dtype=x.dtype, device=x.device)
    if workspace is None:
        workspace = torch.empty(B * R * N * C, dtype=torch.float32, device=x.device)
    check(lib.afldm_af_resample(ptr(x), ptr(M), ptr(out), ptr(workspace), B, N, C, R, _code(x), stream_ptr()),
          "af_resample")
    return out


def af_resample_hw(x, Mh, Mw, out=None, workspace=None):
    """y = Mh x Mw^T per plane (different matrices along H and W): [B,N,N,C] -> [B,R,R,C]."""
    _dev(x, "x")
    B, N, N2, C = x.shape
    assert N == N2 and Mh.shape == Mw.shape and Mh.shape[1] == N
    R = Mh.shape[0]
    if out is None:
        out = torch.empty((B, R, R, C), dtype=x.dtype, device=x.device)
    if workspace is None:
        workspace = torch.empty(B * R * N * C, dtype=torch.float32, device=x.device)
    check(lib.afldm_af_resample_hw(ptr(x), ptr(Mh), ptr(Mw), ptr(out), ptr(workspace), B, N, C, R, _code(x),
                                   stream_ptr()), "af_resample_hw")
    return out


def masked_metrics(a, b, mask):
    """afldm_masked_metrics: [B, 6] fp32 = per-sample (sum ((a-b) m)^2, sum m, max a m, min a m, max b m, min b m)."""
    _dev(a, "a")
    assert a.shape == b.shape
    if a.dtype not in (torch.float32, torch.bfloat16) or b.dtype != a.dtype:
        a, b = a.float(), b.float()
    a, b = a.contiguous(), b.contiguous()
    mask = mask.to(device=a.device, dtype=torch.float32)
    m = mask.expand_as(a).contiguous()
    B = a.shape[0]
    out = torch.empty((B, 6), dtype=torch.float32, device=a.device)
    check(lib.afldm_masked_metrics(ptr(a), ptr(b), ptr(m), ptr(out), B, a.numel() // B, _code(a), stream_ptr()),
          "masked_metrics")
    # The reference divides by mask.sum((1,2,3)) of the mask's OWN shape (metrics.py:6-7): a broadcast
    # [B,1,H,W] mask (what ImageShifter returns) counts each pixel once, not once per channel.  The kernel
    # summed the expanded mask: `rep` copies of every mask element.
    if mask.ndim == a.ndim:
        rep = (a.numel() // B) // max(mask.numel() // mask.shape[0], 1)
        if rep > 1:
            out[:, 1] /= rep
    return out


# ----------------------------------------------------------------------------- upfirdn2d (NCHW planes)
def upfirdn2d(x, f, upx=1, upy=1, downx=1, downy=1, padx0=0, padx1=0, pady0=0, pady1=0, flip_filter=False, gain=1.0,
              out=None):
    """afldm_upfirdn2d on an NCHW CUDA tensor (fp32 / bf16) with a 2-D device fp32 filter [fh, fw]."""
    _dev(x, "x")
    _dev(f, "f")
    assert x.ndim == 4 and f.ndim == 2 and f.dtype == torch.float32
    B, C, H, W = x.shape
    fh, fw = f.shape
    outW = lib.afldm_upfirdn2d_out_size(W, upx, downx, padx0, padx1, fw)
    outH = lib.afldm_upfirdn2d_out_size(H, upy, downy, pady0, pady1, fh)
    assert outW > 0 and outH > 0, "upfirdn2d: the padded / cropped up-sampled plane is smaller than the filter"
    if out is None:
        out = torch.empty((B, C, outH, outW), dtype=x.dtype, device=x.device)
    if B * C == 0:
        return out
    tok = _begin()
    check(lib.afldm_upfirdn2d(ptr(x), ptr(f), ptr(out), B * C, H, W, fh, fw, upx, upy, downx, downy, padx0, padx1,
                              pady0, pady1, int(bool(flip_filter)), float(gain), _code(x), stream_ptr()), "upfirdn2d")
    _end(tok, "upfirdn2d", 2.0 * out.numel() * ((fh + upy - 1) // upy) * ((fw + upx - 1) // upx),
         (x.numel() + out.numel()) * x.element_size())
    return out


# ----------------------------------------------------------------------------- conv / linear
_SYNC = {}
_SYNC_SPARE = {}


SYNC_WORDS = 32768        # int32 words of a sync buffer: [0, 8192) split-K tile counters, [8192] split-K error word, [8193] error word
                          # of the in-launch hand-overs (attention phase C, merged launches: 1 = gave up waiting, 2 = cluster
                          # straddles XCDs, 3 = a barrier of the experimental cooperative trunk timed out), [8200, 8201] that
                          # trunk's grid barrier, [16384, 32768) hand-over counters (one 128-byte line per sample)
_SYNC_OVERRIDE = None
_SCOPED_SYNC = []


def new_sync_buffer(device):
    """A private, zeroed sync buffer (see _sync_words) for ONE stream of launches - a DenoiseEngine (each of its
    branches) owns one, so that graphs captured on torch's shared capture stream and later replayed CONCURRENTLY on
    different streams never share counters."""
    buf = torch.zeros(SYNC_WORDS, dtype=torch.int32, device=device)
    import weakref
    _SCOPED_SYNC[:] = [r for r in _SCOPED_SYNC if r() is not None]
    _SCOPED_SYNC.append(weakref.ref(buf))
    return buf


class sync_scope:
    """with sync_scope(buf): every launch issued inside takes `buf` as its sync words instead of the per-stream one."""

    def __init__(self, buf):
        self.buf = buf

    def __enter__(self):
        global _SYNC_OVERRIDE
        self.prev, _SYNC_OVERRIDE = _SYNC_OVERRIDE, self.buf
        return self.buf

    def __exit__(self, *a):
        global _SYNC_OVERRIDE
        _SYNC_OVERRIDE = self.prev


def _sync_words(device):
    """Zero-initialised counter words for the in-kernel split-K reduction (afldm_conv_args.sync) and the cluster
    hand-overs of the merged launches: one buffer per (device, stream) - launches of ONE stream share it in stream order
    and each leaves it zero; concurrent streams (DenoiseEngine branches) must not share counters.  An
    engine scopes its own buffer over its launches (sync_scope): captured graphs all run on torch's one capture stream
    at capture time but may replay concurrently later."""
    if _SYNC_OVERRIDE is not None:
        return _SYNC_OVERRIDE
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    if key not in _SYNC:
        # never allocate under graph capture (the buffer would live in that graph's private pool while this dict hands
        # it to later graphs and eager launches): streams first seen during a capture - torch's capture
        # stream, the engine's branch streams - take a buffer from a spare list filled on the first eager call
        spares = _SYNC_SPARE.setdefault(str(device), [])
        if torch.cuda.is_current_stream_capturing():
            if not spares:
                raise RuntimeError("afldm_amd: no pre-allocated sync buffer left for a stream first seen under graph "
                                   "capture; run one eager step (warm-up) before capturing")
            _SYNC[key] = spares.pop()
        else:
            _SYNC[key] = new_sync_buffer(device)
            while len(spares) < 8:
                spares.append(new_sync_buffer(device))
    return _SYNC[key]


def fused_splitk_error(device=None):
    """True if an in-kernel split-K reduction (AFLDM_FUSED_SPLITK) gave up waiting for a slice since the last call;
    reads and clears the error word of every sync buffer of the device (synchronises)."""
    hit = False
    for (dev, _), buf in _SYNC.items():
        if device is None or dev == str(device):
            if int(buf[8192].item()):
                hit = True
                buf[8192] = 0
    return hit


def conv_args(x1, w, bias=None, x2=None, temb=None, temb_stride=0, residual=None, out=None, out_mode=0,
              workspace=None, y_ld=None, out2=None, split_n=0, temb_mod=0):
    """Build the afldm_conv_args struct (keeps references to the tensors alive in `.keep`)."""
    C1, x2, C2 = _cat_args(x1, x2)
    _dev(w, "w")
    Cout, KS = w.shape[0], w.shape[1]
    assert w.shape[3] == C1 + C2, f"weight Cin {w.shape[3]} != {C1}+{C2}"
    if x1.ndim == 4:
        B, H, W_ = x1.shape[:3]
    else:                      # [rows, C] or [B, T, C]: a linear layer
        B, H, W_ = x1.numel() // C1, 1, 1
    a = ConvArgs()
    a.x1, a.x2, a.w, a.bias = ptr(x1), ptr(x2), ptr(w), ptr(bias)
    a.temb, a.residual, a.y = ptr(temb), ptr(residual), ptr(out)
    a.workspace = ptr(workspace)
    a.workspace_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    a.C1, a.C2, a.B, a.H, a.W, a.Cout, a.KS = C1, C2, B, H, W_, Cout, KS
    a.temb_stride = int(temb_stride)
    a.res_ld = Cout if residual is None else residual.shape[-1]
    a.y_ld = Cout if y_ld is None else int(y_ld)
    a.out_mode = int(out_mode)
    a.dtype = _code(x1)
    a.y2, a.split_n = ptr(out2), int(split_n)
    a.temb_mod = int(temb_mod)
    if out2 is not None and y_ld is None:
        a.y_ld = int(split_n)
    sync = _sync_words(x1.device)
    a.sync, a.sync_bytes = ptr(sync), sync.numel() * 4
    a.keep = (x1, x2, w, bias, temb, residual, out, workspace, sync)
    a.x_layout = 1 if is_c8(x1) else 0
    assert not is_c8(x2) and not is_c8(residual), "8-channel-block tensors are convolution inputs only"
    return a


_CONV_NORM = os.environ.get("AFLDM_NO_CONV_NORM", "0") != "1"


def conv2d_c8_ok(x1, w, bias=None, temb=None, temb_stride=0, residual=None, want_stats=True):
    """True when afldm_conv2d on this problem reads / writes 8-channel blocks (one halo-patch launch, bf16, 16^2 / 32^2).
    The probe carries what the real launch will carry - the time-embedding stride and a statistics output (the blocked layouts
    need the statistics formed in the epilogue, which depends on both: ADVICE r05)."""
    if not _C8 or x1.ndim != 4 or x1.dtype != torch.bfloat16 or x1.shape[1] != x1.shape[2] or x1.shape[1] not in (16, 32):
        return False
    key = (tuple(x1.shape), tuple(w.shape), temb is not None, int(temb_stride), residual is not None, bool(want_stats), str(x1.device))
    if key not in _C8_OK:
        a = conv_args(x1, w, bias, None, temb, temb_stride, residual, None)
        a.y = ptr(x1)                 # (a non-NULL, aligned placeholder: the queries do not dereference it)
        if want_stats and w.shape[0] % 4 == 0:
            a.stats_out = ptr(x1)
        a.x_layout = 0
        # (a plan that would split K given the room is not the one-launch halo kernel)
        _C8_OK[key] = (not lib.afldm_conv2d_workspace(ctypes.byref(a))) and bool(lib.afldm_conv2d_c8_ok(ctypes.byref(a)))
    return _C8_OK[key]


_C8_OK = {}


def _set_shortcut(a, shortcut):
    sx1, sx2, sw = shortcut
    _dev(sx1, "shortcut x1")
    assert not is_c8(sx1) and not is_c8(sx2), "the folded shortcut reads NHWC tensors"
    a.sc_x1, a.sc_x2, a.sc_w = ptr(sx1), ptr(sx2), ptr(sw)
    a.sc_C1, a.sc_C2 = sx1.shape[-1], 0 if sx2 is None else sx2.shape[-1]
    a.keep = a.keep + (sx1, sx2, sw)


def conv2d_shortcut_ok(x1, w, bias, shortcut, temb=None, temb_stride=0, want_stats=True, slabs=False):
    """Non-zero when conv2d(x1, w, bias, shortcut=(sx1, sx2, sw)) - slabs: conv2d_slabs(x1, w, shortcut=...) - runs the 1x1
    shortcut inside the 3x3 convolution itself (afldm_conv2d_shortcut_ok): 1 on a halo-patch tile with one filter tap per K step
    (whole K per workgroup), 2 on one with three taps per step (the 8^2 / 4^2 levels, the small batches; K may be split there).
    The probe carries what the real launch carries, the split-K workspace included."""
    sx1, sx2, sw = shortcut
    if x1.ndim != 4 or sx1.ndim != 4 or w.shape[1] != 3 or sw.shape[1] != 1:
        return 0
    key = (tuple(x1.shape), is_c8(x1), x1.dtype, tuple(w.shape), tuple(sx1.shape), None if sx2 is None else tuple(sx2.shape),
           temb is not None, int(temb_stride), bool(want_stats), bool(slabs), str(x1.device))
    if key not in _SC_OK:
        a = conv_args(x1, w, None if slabs else bias, None, temb, temb_stride, None, None)
        a.y = ptr(sx1)                 # (a non-NULL, aligned placeholder: the queries do not dereference it)
        if want_stats and not slabs and w.shape[0] % 4 == 0:
            a.stats_out = ptr(sx1)
        _set_shortcut(a, shortcut)
        need = lib.afldm_conv2d_workspace(ctypes.byref(a))
        if need:                       # (the plan splits K when it is given the room, as conv2d / conv2d_slabs give it)
            a.workspace, a.workspace_bytes = ptr(sx1), need
        a.defer_reduce = 1 if slabs else 0
        _SC_OK[key] = int(lib.afldm_conv2d_shortcut_ok(ctypes.byref(a))) if (need or not slabs) else 0
    return _SC_OK[key]


_SC_OK = {}


def conv2d(x1, w, bias=None, x2=None, temb=None, temb_stride=0, residual=None, out=None, out_mode=0,
           workspace=None, want_stats=False, temb_mod=0, w_batch_stride=0, norm_out=None, out_c8=False, shortcut=None):
    """stride-1 'same' conv (KS in {1,3}) / linear on NHWC input with packed OHWI weights.
    shortcut = (sx1, sx2, sw): a 1x1 convolution of the virtual concat sx1 | sx2 with the packed weight sw, added inside this 3x3
    convolution (bias = the sum of both biases; only where conv2d_shortcut_ok says so).
    out_mode 1 returns the channel-major [B, Cout, H*W] tensor (V^T for attention).
    want_stats: also emit the per-channel GroupNorm partial sums of the output (from the GEMM
    epilogue where possible) and attach them to the returned tensor as `.gn_partial`."""
    Cout = w.shape[0]
    if out is None:
        if out_mode == 0:
            out = torch.empty(tuple(x1.shape[:-1]) + (Cout,), dtype=x1.dtype, device=x1.device)
        else:
            B = x1.shape[0]
            out = torch.empty((B, Cout, x1.numel() // (B * x1.shape[-1])), dtype=x1.dtype, device=x1.device)
    a = conv_args(x1, w, bias, x2, temb, temb_stride, residual, out, out_mode, workspace, temb_mod=temb_mod)
    if out_c8:
        a.y_layout = 1
        out.c8 = True
    a.w_batch_stride = int(w_batch_stride)   # per-sample weights (elements between samples' weight tensors; `w` = sample 0's)
    if shortcut is not None:
        _set_shortcut(a, shortcut)
    if out_mode == 1 and x1.ndim == 3:      # [B, T, C] tokens: treat T as the pixel axis
        a.B, a.H, a.W = x1.shape[0], x1.shape[1], 1
    if workspace is None:
        need = lib.afldm_conv2d_workspace(ctypes.byref(a))
        if need:
            workspace = torch.empty(need // 4, dtype=torch.float32, device=x1.device)
            a.workspace, a.workspace_bytes = ptr(workspace), need
    st = None
    if want_stats and out_mode == 0 and Cout % 4 == 0:
        S = lib.afldm_conv2d_stats_splits(ctypes.byref(a))
        st = torch.empty((a.B, S, Cout, 2), dtype=torch.float32, device=x1.device)
        a.stats_out = ptr(st)
    hn = None
    if norm_out is not None and _CONV_NORM and st is not None:
        # norm_out = (gamma, beta, G, eps) of the GroupNorm that consumes this output next: applied by the convolution's own
        # epilogue where a tile holds a whole sample and whole groups (afldm_conv2d_norm_ok); the result rides on the output
        # as `.norm_applied`
        gamma, beta, G, eps = norm_out
        a.norm_gamma, a.norm_beta, a.norm_groups, a.norm_eps = ptr(gamma), ptr(beta), int(G), float(eps)
        if lib.afldm_conv2d_norm_ok(ctypes.byref(a)):
            hn = torch.empty_like(out)
            a.y_norm = ptr(hn)
            a.keep = a.keep + (hn, gamma, beta)
    tok = _begin()
    check(lib.afldm_conv2d(ctypes.byref(a), stream_ptr()), "conv2d")
    if hn is not None:
        out.norm_applied = hn
    if st is not None:
        if st.shape[1] > _MAX_SPLITS and st.shape[1] % _MAX_SPLITS == 0:
            # one split per 128-pixel tile is 512 per sample on a 256^2 plane: fold before the consumers walk them
            folded = torch.empty((a.B, _MAX_SPLITS, Cout, 2), dtype=torch.float32, device=x1.device)
            check(lib.afldm_gn_fold(ptr(st), st.shape[1], ptr(folded), _MAX_SPLITS, a.B, Cout, stream_ptr()), "gn_fold")
            st = folded
        out.gn_partial = st
    if tok is not None:
        M, Ct = a.B * a.H * a.W, a.C1 + a.C2
        es = x1.element_size()
        kind = "conv3x3" if a.KS == 3 else ("conv1x1" if a.H * a.W > 1 and x1.ndim == 4 else "linear")
        Csc = a.sc_C1 + a.sc_C2 if shortcut is not None else 0
        # algorithmic bytes: input + weights + output (+ the residual read; + the folded shortcut's input and weights), as
        # tools/replay_conv3x3.py counts them
        keep = (a, st, out, workspace)
        _end(tok, kind, 2.0 * M * a.Cout * (a.KS * a.KS * Ct + Csc),
             (M * (Ct + Csc) + a.Cout * (a.KS * a.KS * Ct + Csc) + M * a.Cout * (2 if residual is not None else 1)) * es,
             replay=lambda keep=keep: conv2d_launch(keep[0]))
    return out


_ACTCONV = os.environ.get("AFLDM_NO_ACTCONV", "0") != "1"


def act_conv_act(x1, x2, pre, w, bias=None, temb=None, temb_stride=0, residual=None, want_stats=False, post=None):
    """[pre: GroupNorm-apply -> WarpedNonlinearity(SiLU) ->] 3x3 conv [-> post: GroupNorm-apply -> WarpedNonlinearity] as
    ONE launch (afldm_act_conv_act, csrc/actconv.hip).
      pre  = None (x1 IS the convolution's input) or (stats, gamma, beta, G, eps) applied to the virtual concat x1 | x2
             (stats None: activation without normalisation);
      post = None or (gamma, beta, G, eps): the activation of the convolution's own output with the statistics its
             epilogue writes (gamma None: no normalisation).
    Returns (conv_out, post_out) - conv_out carries `.gn_partial` when want_stats or post needs them and `.act_input`
    (the activated input) when pre is given - or None when there is no merged kernel for the chain (the caller runs the
    separate ops).  Bit-identical to them."""
    if (not _ACTCONV or not _exp.available() or x1.ndim != 4 or x1.dtype != torch.bfloat16 or x1.shape[1] != x1.shape[2] or x1.shape[1] not in (16, 32)
            or (pre is None and post is None)):
        return None
    C1, x2, C2 = _cat_args(x1, x2)
    B, N = x1.shape[0], x1.shape[1]
    Cout = w.shape[0]
    if w.shape[1] != 3 or w.shape[3] != C1 + C2 or (pre is None and x2 is not None):
        return None
    act_out = torch.empty((B, N, N, C1 + C2), dtype=x1.dtype, device=x1.device) if pre is not None else x1
    out = torch.empty((B, N, N, Cout), dtype=x1.dtype, device=x1.device)
    a = conv_args(act_out, w, bias, None, temb, temb_stride, residual, out)
    if a.sync_bytes < (16384 + 64 * B) * 4:
        return None
    need = lib.afldm_conv2d_workspace(ctypes.byref(a))
    workspace = None
    if need:                                   # (the plan would split K given the room: no merged kernel then, as conv2d decides)
        workspace = torch.empty(need // 4, dtype=torch.float32, device=x1.device)
        a.workspace, a.workspace_bytes = ptr(workspace), need
    st = None
    post_norm = post is not None and post[0] is not None
    if (want_stats or post_norm) and Cout % 4 == 0:
        S = lib.afldm_conv2d_stats_splits(ctypes.byref(a))
        st = torch.empty((B, S, Cout, 2), dtype=torch.float32, device=x1.device)
        a.stats_out = ptr(st)
    U, D = filter_matrices(N, x1.device)
    packed = packed_filters(N, x1.dtype, x1.device)
    aa = pp = None
    keep = [a, x1, x2, U, D, packed, act_out, out, st, workspace]
    if pre is not None:
        stats, gamma, beta, G, eps = pre
        aa = AfActArgs()
        aa.x1, aa.x2, aa.C1, aa.C2 = ptr(x1), ptr(x2), C1, C2
        p1, S1, p2, S2 = _stats_ptrs(stats)
        aa.stats1, aa.S1, aa.stats2, aa.S2 = p1, S1, p2, S2
        aa.gamma, aa.beta, aa.G, aa.eps = ptr(gamma), ptr(beta), int(G), float(eps)
        aa.U, aa.D, aa.packed = ptr(U), ptr(D), ptr(packed)
        keep += [aa, stats, gamma, beta]
    post_out = None
    if post is not None:
        gamma2, beta2, G2, eps2 = post
        if post_norm and st is None:
            return None
        pp = AfActArgs()
        pp.x1, pp.x2, pp.C1, pp.C2 = ptr(out), None, Cout, 0
        pp.stats1, pp.S1, pp.stats2, pp.S2 = (ptr(st), st.shape[1], None, 0) if post_norm else (None, 0, None, 0)
        pp.gamma, pp.beta, pp.G, pp.eps = ptr(gamma2), ptr(beta2), int(G2), float(eps2)
        pp.U, pp.D, pp.packed = ptr(U), ptr(D), ptr(packed)
        post_out = torch.empty((B, N, N, Cout), dtype=x1.dtype, device=x1.device)
        keep += [pp, gamma2, beta2, post_out]
    ra = ctypes.byref(aa) if aa is not None else None
    rp = ctypes.byref(pp) if pp is not None else None
    if not _exp.lib().afldm_act_conv_act_merged(ra, ctypes.byref(a), rp):
        return None
    keep = tuple(keep)
    tok = _begin()
    check(_exp.lib().afldm_act_conv_act(ra, ctypes.byref(a), rp, ptr(post_out), stream_ptr()), "act_conv_act")
    if st is not None:
        out.gn_partial = st
    if tok is not None:
        M, Ct, es = B * N * N, C1 + C2, x1.element_size()
        # algorithmic work of the chain: the activations' dense separable form + the convolution; bytes: every tensor the
        # separate launches would read / write once (raw in, activated in, weights, output (+ residual), activated out)
        fl = 2.0 * M * Cout * 9 * Ct + (24.0 * N ** 3 * B * Ct if pre is not None else 0.0) + (24.0 * N ** 3 * B * Cout if post is not None else 0.0)
        by = (M * Ct * (2 if pre is not None else 1) + Cout * 9 * Ct + M * Cout * ((2 if residual is not None else 1) + (1 if post is not None else 0))) * es
        name = ("af_act_" if pre is not None else "") + "conv3x3" + ("_af_act" if post is not None else "") + f"_N{N}"

        def replay(ra=ra, rp=rp, a=a, post_out=post_out, keep=keep):
            check(_exp.lib().afldm_act_conv_act(ra, ctypes.byref(a), rp, ptr(post_out), stream_ptr()), "act_conv_act")
        _end(tok, name, fl, by, replay=replay)
    if pre is not None:
        out.act_input = act_out          # the activated tensor (kept alive with the output; tests read it)
    return out, post_out


def af_act_conv2d(x1, x2, stats, gamma, beta, G, eps, w, bias=None, temb=None, temb_stride=0, residual=None,
                  want_stats=False):
    """[GroupNorm-apply ->] WarpedNonlinearity(SiLU) -> 3x3 conv as ONE launch: act_conv_act without the trailing
    activation.  Returns the convolution's output or None (no merged kernel: the caller runs af_act + conv2d)."""
    got = act_conv_act(x1, x2, (stats, gamma, beta, G, eps), w, bias, temb, temb_stride, residual, want_stats)
    return None if got is None else got[0]


def actconv_error(device=None):
    """Error word of the merged launches' cluster hand-over (0 = fine; 1 = a workgroup gave up waiting for its cluster,
    2 = a workgroup did not run on the XCD its id implies) over every sync buffer seen so far; synchronises, clears."""
    worst = 0
    bufs = [b for (dev, _), b in _SYNC.items() if device is None or dev == str(device)] + [r() for r in _SCOPED_SYNC if r() is not None]
    for buf in bufs:
        v = int(buf[8193].item())
        if v:
            worst = max(worst, v)
            buf[8193] = 0
    return worst


def conv2d_slabs(x1, w, x2=None, shortcut=None):
    """The split-K slabs of conv2d(x1 | x2, w) WITHOUT the reduction launch (afldm_conv_args.defer_reduce): returns
    (slabs fp32 [nslab, M, Cout], nslab), or None when the plan for this shape does not split K (the caller then runs
    the ordinary conv2d).  Bias, time embedding and residual are NOT applied: the consumer (af_act_slabs) adds them.
    shortcut = (sx1, sx2, sw): the slabs carry conv3x3 + the folded 1x1 shortcut (conv2d_shortcut_ok(..., slabs=True));
    the consumer then takes the sum of both biases and no residual."""
    Cout = w.shape[0]
    out = torch.empty(tuple(x1.shape[:-1]) + (Cout,), dtype=x1.dtype, device=x1.device)      # (never written when K is split)
    a = conv_args(x1, w, None, x2, out=out)
    if shortcut is not None:
        _set_shortcut(a, shortcut)
    need = lib.afldm_conv2d_workspace(ctypes.byref(a))
    if not need:
        return None
    workspace = torch.empty(need // 4, dtype=torch.float32, device=x1.device)
    a.workspace, a.workspace_bytes = ptr(workspace), need            # (the plan only splits K when it is given the room)
    code = lib.afldm_conv2d_variant(ctypes.byref(a))
    nslab = (code >> 8) & 255 if code >= 0 else 1
    if code < 0 or nslab <= 1 or (code >> 16) & 1 or need < nslab * a.B * a.H * a.W * Cout * 4:
        return None
    a.defer_reduce = 1
    a.keep = a.keep + (workspace,)
    tok = _begin()
    check(lib.afldm_conv2d(ctypes.byref(a), stream_ptr()), "conv2d(slabs)")
    if tok is not None:
        M, Ct = a.B * a.H * a.W, a.C1 + a.C2
        es = x1.element_size()
        kind = "conv3x3" if a.KS == 3 else ("conv1x1" if a.H * a.W > 1 and x1.ndim == 4 else "linear")
        keep = (a, workspace, out)
        Csc = a.sc_C1 + a.sc_C2 if shortcut is not None else 0
        _end(tok, kind, 2.0 * M * a.Cout * (a.KS * a.KS * Ct + Csc), (M * (Ct + Csc) + a.Cout * (a.KS * a.KS * Ct + Csc) + M * a.Cout) * es,
             replay=lambda keep=keep: conv2d_launch(keep[0]))
    return workspace[:nslab * a.B * a.H * a.W * Cout].view(nslab, a.B * a.H * a.W, Cout), nslab


def af_act_slabs(slabs, nslab, bias, temb, temb_stride, gamma, beta, G, eps, B, N, C, dtype, residual=None, want_raw=False,
                 act=True):
    """A convolution's split-K slabs straight into the following GroupNorm on 2x2 / 4x4 planes (afldm_af_act_slabs):
    act=True -> GroupNorm + WarpedNonlinearity (conv1 -> norm2 of a resnet), act=False -> GroupNorm only (conv2 ->
    Attention.group_norm).  Returns the [B, N, N, C] result, or (result, raw) with the finished convolution output
    itself when want_raw."""
    const = act == 2       # N = 2: the plane-constant activation stored once, [B, C] tagged `.const2` (af_act out_const)
    assert not const or N == 2
    out = torch.empty((B, C) if const else (B, N, N, C), dtype=dtype, device=slabs.device)
    raw = torch.empty((B, N, N, C), dtype=dtype, device=slabs.device) if want_raw else None
    U, D = filter_matrices(N, slabs.device)
    tok = _begin()
    check(lib.afldm_af_act_slabs(ptr(slabs), int(nslab), ptr(bias), ptr(temb), int(temb_stride), ptr(residual), ptr(raw),
                                 ptr(gamma), ptr(beta), int(G), float(eps), 2 if const else (1 if act else 0), ptr(U), ptr(D),
                                 ptr(out), B, C, N, _code(out), stream_ptr()), "af_act_slabs")
    if const:
        out.const2 = True
    _end(tok, f"af_act_N{N}" if act else "gn_apply", 24.0 * N ** 3 * B * C if act else 0.0,
         B * N * N * C * (4 * nslab + out.element_size() * (2 if want_raw else 1)))
    return (out, raw) if want_raw else out


# smallest batch the fused conv1 -> norm2 -> activation launch of the 2x2 level is used for: a workgroup owns a whole GroupNorm group
# (96 weight rows x all of K = 147 - 295 KB, which one CU pulls at ~30 GB/s whatever the order of the workgroups), i.e. 32 workgroups
# per 16 samples.  Same-box, alternating, ms/step with / without: batch 64 4.610 / 4.637, 4.628 / 4.664, 4.823 / 4.843 (three boxes);
# batch 32 3.217 / 3.202, 3.268 / 3.247; batch 16 2.620 / 2.600; batch 8 2.298 / 2.290; batch 1 2.026 / 2.002
# (profiles/r06/ab_dense2_r06c.log, ab_skinny_dense2_policy_r06d.log, ab_dense2_xcd_r06e.log): k_skinny's 192 x 24 KB wins below 64
_DENSE2_MIN_B = int(os.environ.get("AFLDM_DENSE2_MIN_B", "64"))


def conv2x2_const_norm_act_ok(Cin, Cout, G, dtype, batch=None):
    """True when afldm_conv2x2_const_norm_act has a kernel for the shape and (batch given) the policy picks it."""
    if batch is not None and batch < _DENSE2_MIN_B:
        return False
    return bool(lib.afldm_conv2x2_const_norm_act_supported(int(Cin), int(Cout), int(G), DTYPE_CODE[dtype]))


def conv2x2_const_norm_act(a, w_cm, bias, temb, temb_stride, gamma, beta, G, eps):
    """conv1 + temb -> norm2 -> WarpedNonlinearity of a ResnetBlock2D on 2x2 planes in ONE launch (afldm_conv2x2_const_norm_act):
    a [B, Cin] the plane-constant first activation, w_cm [4 Cout, 1, 1, Cin] the tap-summed dense weights with channel-major rows
    (row = 4 n + pixel), bias [Cout] fp32, temb the block's time_emb_proj slice.  Returns the plane-constant second activation
    [B, Cout] (tagged `.const2`)."""
    _dev(a, "a")
    B, Cin = a.shape
    Cout = w_cm.shape[0] // 4
    out = torch.empty((B, Cout), dtype=a.dtype, device=a.device)
    U, D = filter_matrices(2, a.device)
    tok = _begin()
    check(lib.afldm_conv2x2_const_norm_act(ptr(a), ptr(w_cm), ptr(bias), ptr(temb), int(temb_stride), ptr(gamma), ptr(beta), int(G),
                                           float(eps), ptr(U), ptr(D), ptr(out), B, Cin, Cout, _code(a), stream_ptr()),
          "conv2x2_const_norm_act")
    _end(tok, "linear", 2.0 * B * 4 * Cout * Cin, (B * Cin + 4 * Cout * Cin + B * Cout) * a.element_size())
    out.const2 = True
    return out


def conv_out_fused(x, w, bias, gamma, beta, G, eps):
    """conv_norm_out -> SiLU -> conv_out (3x3, <= 4 couts) of the UNet tail in one launch (afldm_conv_out_fused);
    returns None when the shape is not covered (the caller runs gn_apply + conv2d)."""
    if (x.dtype != torch.bfloat16 or x.ndim != 4 or x.shape[1] != 32 or x.shape[2] != 32 or x.shape[3] not in (64, 128, 192)
            or w.shape[0] > 4 or w.shape[1] != 3 or os.environ.get("AFLDM_NO_CONV_OUT_FUSED")
            or G > 64 or G <= 0 or x.shape[3] % G or not x.is_contiguous()):      # the C side's own constraints
        return None
    B, N, _, C = x.shape
    Cout = w.shape[0]
    st = _tensor_stats(x, None)
    out = torch.empty((B, N, N, Cout), dtype=x.dtype, device=x.device)
    tok = _begin()
    check(lib.afldm_conv_out_fused(ptr(x), ptr(st), st.shape[1], ptr(gamma), ptr(beta), int(G), float(eps), ptr(w), ptr(bias),
                                   ptr(out), B, N, C, Cout, _code(x), stream_ptr()), "conv_out_fused")
    _end(tok, "conv_out", 2.0 * B * N * N * Cout * 9 * C, (B * N * N * (C + Cout) + Cout * 9 * C) * x.element_size())
    return out


def conv_workspace_bytes(a):
    return lib.afldm_conv2d_workspace(ctypes.byref(a))


def linear_split(x, w, bias, split_n, workspace=None):
    """One GEMM over tokens x [B, T, C] with weight rows [0, split_n) -> token-major [B, T, split_n]
    and rows [split_n, Cout) -> channel-major [B, Cout - split_n, T] (fused Q|K|V projection)."""
    _dev(x, "x")
    B, T, C = x.shape
    Cout = w.shape[0]
    y = torch.empty((B, T, split_n), dtype=x.dtype, device=x.device)
    y2 = torch.empty((B, Cout - split_n, T), dtype=x.dtype, device=x.device)
    a = conv_args(x, w, bias, out=y, out2=y2, split_n=split_n)
    a.B, a.H, a.W = B, T, 1
    if workspace is None:
        need = lib.afldm_conv2d_workspace(ctypes.byref(a))
        if need:
            workspace = torch.empty(need // 4, dtype=torch.float32, device=x.device)
            a.workspace, a.workspace_bytes = ptr(workspace), need
    tok = _begin()
    check(lib.afldm_conv2d(ctypes.byref(a), stream_ptr()), "conv2d(split)")
    _end(tok, "linear", 2.0 * B * T * Cout * C, (B * T * C + Cout * C + B * T * Cout) * x.element_size())
    return y, y2


def conv2d_launch(a):
    check(lib.afldm_conv2d(ctypes.byref(a), stream_ptr()), "conv2d")


# ----------------------------------------------------------------------------- vanilla resamplers (csrc/resconv.hip)
def fold_up2_weight(w):
    """conv3x3(nearest2x(x)) as four 2x2 convolutions of x: OIHW [Cout, Cin, 3, 3] -> [4, Cout, Cin, 2, 2] fp32, phase
    p = 2 a + c computes output pixel (2i + a, 2j + c) from input rows {i - 1 + a, i + a} and columns {j - 1 + c, j + c}.
    Per axis, phase 0 takes taps {w0, w1 + w2} and phase 1 {w0 + w1, w2}; rows are folded first, then columns (the order
    afldm_pack_weight_up2 sums in, so the two agree bit for bit)."""
    w = w.detach().to(torch.float32)
    rows = [torch.stack([w[:, :, 0], w[:, :, 1] + w[:, :, 2]], 2),          # [Cout, Cin, 2, 3] per row phase
            torch.stack([w[:, :, 0] + w[:, :, 1], w[:, :, 2]], 2)]
    out = []
    for a in (0, 1):
        r = rows[a]
        for cols in ((r[..., 0], r[..., 1] + r[..., 2]), (r[..., 0] + r[..., 1], r[..., 2])):
            out.append(torch.stack(cols, 3))
    return torch.stack(out, 0).contiguous()


def pack_weight_up2(w, dtype):
    """OIHW fp32 [Cout, Cin, 3, 3] -> the folded weight [4, Cout, 2, 2, Cin] of conv2d_up2 in `dtype` (one rounding)."""
    _dev(w, "weight")
    w = w.detach().to(torch.float32).contiguous()
    Cout, Cin, KH, KW = w.shape
    assert (KH, KW) == (3, 3), "the nearest-x2 fold is defined for 3x3 kernels"
    out = torch.empty((4, Cout, 2, 2, Cin), dtype=dtype, device=w.device)
    check(lib.afldm_pack_weight_up2(ptr(w), ptr(out), Cout, Cin, _code(out), stream_ptr()), "pack_weight_up2")
    return out


def _resconv_args(x, w, bias, out, Cout):
    _dev(x, "x")
    _dev(w, "w")
    if bias is not None:
        _dev(bias, "bias")
    a = ConvArgs()
    a.x1, a.w, a.bias, a.y = ptr(x), ptr(w), ptr(bias), ptr(out)
    a.B, a.H, a.W = x.shape[:3]
    a.C1, a.Cout, a.KS = x.shape[-1], Cout, 3
    a.y_ld = a.res_ld = Cout
    a.dtype = _code(x)
    a.keep = (x, w, bias, out)
    return a


def _resconv_stats(out, a, S):
    st = torch.empty((a.B, S, a.Cout, 2), dtype=torch.float32, device=out.device)
    a.stats_out = ptr(st)
    a.keep = a.keep + (st,)
    return st


def _fold_stats(st, B, Cout, device):
    if st.shape[1] > _MAX_SPLITS and st.shape[1] % _MAX_SPLITS == 0:
        folded = torch.empty((B, _MAX_SPLITS, Cout, 2), dtype=torch.float32, device=device)
        check(lib.afldm_gn_fold(ptr(st), st.shape[1], ptr(folded), _MAX_SPLITS, B, Cout, stream_ptr()), "gn_fold")
        return folded
    return st


def conv2d_s2(x, w, bias=None, pad=(1, 1), want_stats=False, out=None):
    """F.conv2d(x, w, bias, stride=2) of x zero-padded by pad = (pad_lo, pad_hi) rows / columns, NHWC [B, H, W, Cin] ->
    [B, H/2, W/2, Cout] (afldm_conv2d_s2).  w: the packed OHWI weight (pack_weight).  Downsample2D uses pad (1, 1), the VAE
    encoder's F.pad(x, (0, 1, 0, 1)) + padding=0 is (0, 1).  want_stats: the output carries its GroupNorm partial sums
    (.gn_partial) from the epilogue."""
    B, H, W_, _ = x.shape
    Cout = w.shape[0]
    assert tuple(w.shape[1:3]) == (3, 3) and w.shape[3] == x.shape[-1], f"weight {tuple(w.shape)} vs input {tuple(x.shape)}"
    if out is None:
        out = torch.empty((B, H // 2, W_ // 2, Cout), dtype=x.dtype, device=x.device)
    a = _resconv_args(x, w, bias, out, Cout)
    st = _resconv_stats(out, a, lib.afldm_conv2d_s2_stats_splits(ctypes.byref(a))) if want_stats else None
    lo, hi = int(pad[0]), int(pad[1])
    tok = _begin()
    check(lib.afldm_conv2d_s2(ctypes.byref(a), lo, hi, stream_ptr()), "conv2d_s2")
    if st is not None:
        out.gn_partial = _fold_stats(st, B, Cout, x.device)
    if tok is not None:
        M, Cin = B * (H // 2) * (W_ // 2), x.shape[-1]
        _end(tok, "conv_s2", 2.0 * M * Cout * 9 * Cin, (B * H * W_ * Cin + Cout * 9 * Cin + M * Cout) * x.element_size(),
             replay=lambda a=a: check(lib.afldm_conv2d_s2(ctypes.byref(a), lo, hi, stream_ptr()), "conv2d_s2"))
    return out


def conv2d_up2(x, w_up2, bias=None, want_stats=False, out=None):
    """F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, bias, padding=1) on NHWC [B, H, W, Cin] ->
    [B, 2H, 2W, Cout] without forming the x2 tensor (afldm_conv2d_up2).  w_up2: pack_weight_up2(w).  Profiled FLOPs are
    the folded ones (16 taps per 2x2 output block); the literal convolution does 36."""
    B, H, W_, Cin = x.shape
    assert w_up2.ndim == 5 and w_up2.shape[0] == 4 and w_up2.shape[4] == Cin, f"weight {tuple(w_up2.shape)} vs {tuple(x.shape)}"
    Cout = w_up2.shape[1]
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W_, Cout), dtype=x.dtype, device=x.device)
    a = _resconv_args(x, w_up2, bias, out, Cout)
    st = _resconv_stats(out, a, lib.afldm_conv2d_up2_stats_splits(ctypes.byref(a))) if want_stats else None
    tok = _begin()
    check(lib.afldm_conv2d_up2(ctypes.byref(a), stream_ptr()), "conv2d_up2")
    if st is not None:
        out.gn_partial = _fold_stats(st, B, Cout, x.device)
    if tok is not None:
        M = B * H * W_
        _end(tok, "conv_up2", 2.0 * M * 4 * Cout * 4 * Cin, (M * Cin + 16 * Cout * Cin + 4 * M * Cout) * x.element_size(),
             replay=lambda a=a: check(lib.afldm_conv2d_up2(ctypes.byref(a), stream_ptr()), "conv2d_up2"))
    return out


# ----------------------------------------------------------------------------- attention
def attention(q, k, vt, heads, scale=None, out=None):
    """q [B,Tq,C], k [Bk,Tk,C] token-major (may be column slices of wider buffers: the leading
    dimension is taken from stride(1)); vt [Bk,C,Tk] channel-major; returns [B,Tq,C]."""
    _dev(vt, "vt")
    if not (q.is_cuda and k.is_cuda):
        raise RuntimeError("afldm_amd: attention inputs must live on an MI355X (cuda) device; there is no CPU path")
    B, Tq, C = q.shape
    Bk, Tk, _ = k.shape
    ldq, ldk = q.stride(1), k.stride(1)
    assert q.stride(2) == 1 and k.stride(2) == 1 and q.stride(0) == Tq * ldq and k.stride(0) == Tk * ldk
    d = C // heads
    if scale is None:
        scale = d ** -0.5
    if out is None:
        out = torch.empty((B, Tq, C), dtype=q.dtype, device=q.device)
    tok = _begin()
    check(lib.afldm_attention(ptr(q), ldq, ptr(k), ldk, ptr(vt), ptr(out), C, B, Bk, heads, Tq, Tk, d, float(scale),
                              _code(q), stream_ptr()), "attention")
    _end(tok, "attention", 4.0 * B * heads * Tq * Tk * d, (2 * B * Tq * C + 2 * Bk * Tk * C) * q.element_size())
    return out


def attention_interp(q, k0, vt0, k1, vt1, alpha, heads, scale=None, out=None):
    """(1 - alpha[b]) * attention(q, k0, vt0) + alpha[b] * attention(q, k1, vt1) for every sample b, each softmax normalised on
    its own, blended in fp32 and rounded once (afldm_attention_interp: one launch).  Layouts as attention(); the two sources
    have the same shape and the same leading dimension (k0 / k1 may be column slices of wider buffers).  alpha: fp32 device
    tensor [B], read when the kernel runs - a captured graph picks up the values it holds at each replay."""
    _dev(vt0, "vt0")
    _dev(vt1, "vt1")
    _dev(alpha, "alpha")
    if not (q.is_cuda and k0.is_cuda and k1.is_cuda):
        raise RuntimeError("afldm_amd: attention inputs must live on an MI355X (cuda) device; there is no CPU path")
    B, Tq, C = q.shape
    Bk, Tk, _ = k0.shape
    if k1.shape != k0.shape or k1.stride() != k0.stride() or vt1.shape != vt0.shape or k0.dtype != k1.dtype:
        raise ValueError(f"attention_interp: the two sources differ: k {tuple(k0.shape)} / {tuple(k1.shape)} (strides "
                         f"{k0.stride()} / {k1.stride()}), vt {tuple(vt0.shape)} / {tuple(vt1.shape)}")
    if alpha.dtype != torch.float32 or tuple(alpha.shape) != (B,):
        raise ValueError(f"attention_interp: alpha must be fp32 [{B}], got {alpha.dtype} {tuple(alpha.shape)}")
    ldq, ldk = q.stride(1), k0.stride(1)
    assert q.stride(2) == 1 and k0.stride(2) == 1 and q.stride(0) == Tq * ldq and k0.stride(0) == Tk * ldk
    d = C // heads
    if scale is None:
        scale = d ** -0.5
    if out is None:
        out = torch.empty((B, Tq, C), dtype=q.dtype, device=q.device)
    tok = _begin()
    check(lib.afldm_attention_interp(ptr(q), ldq, ptr(k0), ptr(k1), ldk, ptr(vt0), ptr(vt1), ptr(alpha), ptr(out), C, B, Bk,
                                     heads, Tq, Tk, d, float(scale), _code(q), stream_ptr()), "attention_interp")
    _end(tok, "attention_interp", 8.0 * B * heads * Tq * Tk * d, (2 * B * Tq * C + 4 * Bk * Tk * C) * q.element_size())
    return out


def attention_bank(q, k_bank, vt_bank, src, alpha, heads, scale=None, out=None):
    """attention_interp() with every sample naming its own two sources in a bank: k_bank [S,Tk,C] / vt_bank [S,C,Tk] (layouts as
    attention(); what a STORE pass at batch S leaves), src int32 [B,2] bank slots (clamped into [0, S) by the kernel), alpha
    fp32 [B]; both device tensors, read when the kernel runs - a captured graph picks up the values they hold at each replay.
    A sample with alpha == 0 never reads its second source (afldm_attention_bank: one launch)."""
    _dev(vt_bank, "vt_bank")
    _dev(src, "src")
    _dev(alpha, "alpha")
    if not (q.is_cuda and k_bank.is_cuda):
        raise RuntimeError("afldm_amd: attention inputs must live on an MI355X (cuda) device; there is no CPU path")
    B, Tq, C = q.shape
    S, Tk, _ = k_bank.shape
    if tuple(vt_bank.shape) != (S, C, Tk) or not vt_bank.is_contiguous() or k_bank.dtype != q.dtype or vt_bank.dtype != q.dtype:
        raise ValueError(f"attention_bank: bank k {tuple(k_bank.shape)} {k_bank.dtype} / vt {tuple(vt_bank.shape)} {vt_bank.dtype} "
                         f"(contiguous: {vt_bank.is_contiguous()}) does not match q {tuple(q.shape)} {q.dtype}")
    if src.dtype != torch.int32 or tuple(src.shape) != (B, 2) or not src.is_contiguous():
        raise ValueError(f"attention_bank: src must be contiguous int32 [{B}, 2], got {src.dtype} {tuple(src.shape)}")
    if alpha.dtype != torch.float32 or tuple(alpha.shape) != (B,):
        raise ValueError(f"attention_bank: alpha must be fp32 [{B}], got {alpha.dtype} {tuple(alpha.shape)}")
    ldq, ldk = q.stride(1), k_bank.stride(1)
    assert q.stride(2) == 1 and k_bank.stride(2) == 1 and q.stride(0) == Tq * ldq and k_bank.stride(0) == Tk * ldk
    d = C // heads
    if scale is None:
        scale = d ** -0.5
    if out is None:
        out = torch.empty((B, Tq, C), dtype=q.dtype, device=q.device)
    tok = _begin()
    check(lib.afldm_attention_bank(ptr(q), ldq, ptr(k_bank), ldk, ptr(vt_bank), ptr(src), ptr(alpha), ptr(out), C, B, S, heads, Tq,
                                   Tk, d, float(scale), _code(q), stream_ptr()), "attention_bank")
    _end(tok, "attention_bank", 8.0 * B * heads * Tq * Tk * d, (2 * B * Tq * C + 4 * S * Tk * C) * q.element_size())
    return out


_FUSED_ATTN = os.environ.get("AFLDM_NO_FUSED_ATTN", "0") != "1"
# below this many (sample, head) workgroups the chip is too empty with one workgroup per pair: the three-launch path wins.
# In-step A/B (profiles/r04/small_batch_tiles_ab.txt): 128 against 256: batch 8 2.385 -> 2.362 (the 16^2 level fuses), batch 12
# 2.741 -> 2.710, batch 16 2.741 -> 2.717, batch 24 3.485 -> 3.373 ms/step; 64: batch 8 2.394 (the 32^2 level loses)
_FUSED_ATTN_MIN_WGS = int(os.environ.get("AFLDM_FUSED_ATTN_MIN_WGS", "128"))
# fewest tokens per sample the fused launch is used for (in-step A/B decides between the 32^2 level only and 32^2 + 16^2)
_FUSED_ATTN_MIN_T = int(os.environ.get("AFLDM_FUSED_ATTN_MIN_T", "256"))


def attn_block_fused_ok(x, heads, G):
    """True when afldm_attn_block_fused has a kernel for tokens x [B, T, C] (bf16) and the policy wants it."""
    if not _FUSED_ATTN or x.dtype != torch.bfloat16:
        return False
    B, T, C = x.shape
    if B * heads < _FUSED_ATTN_MIN_WGS or T < _FUSED_ATTN_MIN_T:
        return False
    return bool(lib.afldm_attn_block_fused_supported(T, C, C // heads, int(G)))


# AFLDM_ATTN_FUSED_OUT=0: to_out + residual as its own launch behind the fused front end (A/B; the default carries them in
# the attention launch where afldm_attn_block_fused_out has a kernel: the 32 x 32 level, batch a multiple of 8)
_FUSED_ATTN_OUT = os.environ.get("AFLDM_ATTN_FUSED_OUT", "1") != "0"


_HANDOVER_DEVICES = {}


def handover_device_ok(device):
    """The in-launch hand-over of afldm_attn_block_fused_out relies on the dispatcher dealing consecutive workgroup ids round
    robin to the 8 XCDs of an UNPARTITIONED, UNMASKED MI355X (a sample's 8 head workgroups then share one XCD and its L2):
    256 CUs visible and no CU mask in the environment.  Anything else (a partitioned device, HSA_CU_MASK / ROC_GLOBAL_CU_MASK)
    takes the two-launch path."""
    key = str(device)
    if key not in _HANDOVER_DEVICES:
        masked = any(os.environ.get(v) for v in ("HSA_CU_MASK", "ROC_GLOBAL_CU_MASK", "HSA_CU_MASK_SKIP_INIT"))
        props = torch.cuda.get_device_properties(device)
        _HANDOVER_DEVICES[key] = (not masked) and props.multi_processor_count == 256
    return _HANDOVER_DEVICES[key]


def attn_block_fused_out_ok(x, heads, G):
    B, T, C = x.shape
    return bool(_FUSED_ATTN_OUT and handover_device_ok(x.device)
                and lib.afldm_attn_block_fused_out_supported(B, T, C, C // heads, int(G)))


def sync_errors(bufs, clear=True):
    """(split-K error, hand-over error) over sync buffers: words 8192 / 8193 (see SYNC_WORDS), read with ONE device
    synchronisation per buffer.  A non-zero hand-over word means a launch finished on incomplete data: with `clear` the
    error words AND the hand-over counter lines are zeroed so that later launches start from a clean buffer."""
    sk = ho = 0
    for buf in bufs:
        w = buf[8192:8194].cpu()
        a, b = int(w[0]), int(w[1])
        if (a or b) and clear:
            buf[8192:8194].zero_()
            buf[16384:].zero_()
        sk, ho = max(sk, a), max(ho, b)
    return sk, ho


def attn_block_fused_out(x, stats, gamma, beta, G, eps, w_qkv, bias_qkv, heads, scale, w_out, bias_out):
    """The whole attention block in ONE launch: attn_block_fused + to_out + residual.  Returns y [B, T, C] = to_out(o) + x
    with its GroupNorm partial sums attached (`.gn_partial` [B, heads, C, 2])."""
    _dev(x, "x")
    B, T, C = x.shape
    o = torch.empty_like(x)
    y = torch.empty_like(x)
    st = torch.empty((B, heads, C, 2), dtype=torch.float32, device=x.device)
    sync = _sync_words(x.device)
    assert stats.st2 is None and stats.st1.shape[2] == C
    tok = _begin()
    check(lib.afldm_attn_block_fused_out(ptr(x), ptr(stats.st1), stats.S1, ptr(gamma), ptr(beta), int(G), float(eps),
                                         ptr(w_qkv), ptr(bias_qkv), ptr(o), ptr(w_out), ptr(bias_out), ptr(y), ptr(st),
                                         ptr(sync), sync.numel() * 4, B, T, C, heads, float(scale), _code(x), stream_ptr()),
          "attn_block_fused_out")
    d = C // heads
    _end(tok, "attn_fused", 2.0 * B * T * 4 * C * C + 4.0 * B * heads * T * T * d,
         (3 * B * T * C + 4 * C * C) * x.element_size())
    y.gn_partial = st
    return y


def attn_block_fused(x, stats, gamma, beta, G, eps, w_qkv, bias_qkv, heads, scale, out=None):
    """GroupNorm-apply -> q | k | v projection -> attention of one attention block in ONE launch.  x [B, T, C] raw
    tokens; stats = GNStats of x; w_qkv [3C, 1, 1, C] / bias_qkv [3C] = packed (to_q | to_k | to_v).  Returns the input
    of to_out, [B, T, C]."""
    _dev(x, "x")
    B, T, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    assert stats.st2 is None and stats.st1.shape[2] == C
    tok = _begin()
    check(lib.afldm_attn_block_fused(ptr(x), ptr(stats.st1), stats.S1, ptr(gamma), ptr(beta), int(G), float(eps),
                                     ptr(w_qkv), ptr(bias_qkv), ptr(out), B, T, C, heads, float(scale), _code(x),
                                     stream_ptr()), "attn_block_fused")
    d = C // heads
    _end(tok, "attn_fused", 2.0 * B * T * 3 * C * C + 4.0 * B * heads * T * T * d,
         (2 * B * T * C + 3 * C * C) * x.element_size())
    return out


_ATTN_SMALL = os.environ.get("AFLDM_NO_ATTN_SMALL", "0") != "1"
# token counts the policy sends to the fused small-plane launch.  EMPTY by default: correct (tests) but not faster in the step -
# 4.662 / 4.665 ms without, 4.676 / 4.670 with the 4x4 sites, 4.718 with the 8x8 sites too (profiles/r05/attn_small_ab.txt: on
# its own 20.1 us at 4x4 against 17 + 8, 27.0 against 22.2 at 8x8 where the per-lane VALU attention over 64 keys is 12 us of it).
# AFLDM_ATTN_SMALL_T=16,64 enables it.
_ATTN_SMALL_T = tuple(int(v) for v in os.environ.get("AFLDM_ATTN_SMALL_T", "").split(",") if v)


def attn_small_fused_ok(x, heads):
    """True when afldm_attn_small_fused has a kernel for the (already normalised) tokens x [B, T, C]."""
    if not _ATTN_SMALL or x.dtype != torch.bfloat16 or x.ndim != 3:
        return False
    B, T, C = x.shape
    if T not in _ATTN_SMALL_T:
        return False
    return bool(_exp.lib().afldm_attn_small_fused_supported(B, T, C, int(heads)))


def attn_small_fused(x, w_qkv, bias_qkv, heads, scale, out=None):
    """q | k | v projection + attention of the 8x8 / 4x4 levels in ONE launch; x [B, T, C] = the GroupNorm-ed tokens."""
    _dev(x, "x")
    B, T, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    tok = _begin()
    check(_exp.lib().afldm_attn_small_fused(ptr(x), ptr(w_qkv), ptr(bias_qkv), ptr(out), B, T, C, int(heads), float(scale), _code(x),
                                     stream_ptr()), "attn_small_fused")
    d = C // heads
    _end(tok, "attn_small", 2.0 * B * T * 3 * C * C + 4.0 * B * heads * T * T * d, (2 * B * T * C + 3 * C * C) * x.element_size())
    return out


# ----------------------------------------------------------------------------- DDIM
def ddim_step(x, eps_nhwc, coef, step_idx, advance=False, out=None):
    """x NCHW fp32, eps NHWC dtype; coef float[4*nsteps] and step_idx int32[1] on device."""
    _dev(x, "x"); _dev(eps_nhwc, "eps")
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_ddim_step(ptr(x), ptr(eps_nhwc), ptr(out), ptr(coef), ptr(step_idx), int(advance), B, C, H, W,
                              _code(eps_nhwc), stream_ptr()), "ddim_step")
    return out


def ddim_step_flat(x, eps, coefs, out=None):
    """x, eps: same-shape contiguous fp32 CUDA tensors; coefs = 4 python floats."""
    _dev(x, "x"); _dev(eps, "eps")
    assert x.dtype == eps.dtype == torch.float32 and x.shape == eps.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_ddim_step_flat(ptr(x), ptr(eps), ptr(out), *[float(c) for c in coefs], x.numel(), stream_ptr()),
          "ddim_step_flat")
    return out


# ----------------------------------------------------------------------------- DPM-Solver(++)
def dpm_step(x, eps_nhwc, hist, coef, step_idx, advance=False, out=None):
    """x NCHW fp32, eps NHWC dtype, hist fp32 [2, B, C, H, W] (updated in place); coef float[8*nsteps] and step_idx
    int32[1] on device."""
    _dev(x, "x"); _dev(eps_nhwc, "eps"); _dev(hist, "hist")
    B, C, H, W = x.shape
    assert hist.dtype == torch.float32 and hist.is_contiguous() and tuple(hist.shape) == (2, B, C, H, W)
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_dpm_step(ptr(x), ptr(eps_nhwc), ptr(out), ptr(hist), ptr(coef), ptr(step_idx), int(advance), B, C, H, W,
                             _code(eps_nhwc), stream_ptr()), "dpm_step")
    return out


def dpm_step_flat(x, eps, hist, row, out=None):
    """x, eps: same-shape contiguous fp32 CUDA tensors; hist fp32 [2, *x.shape] (updated in place); row = the six
    floats (p, q, a, b0, b1, b2)."""
    _dev(x, "x"); _dev(eps, "eps"); _dev(hist, "hist")
    assert x.dtype == eps.dtype == hist.dtype == torch.float32 and x.shape == eps.shape and hist.is_contiguous()
    assert hist.numel() == 2 * x.numel()
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_dpm_step_flat(ptr(x), ptr(eps), ptr(out), ptr(hist), *[float(c) for c in row[:6]], x.numel(),
                                  stream_ptr()), "dpm_step_flat")
    return out


# ----------------------------------------------------------------------------- the step updates' shared checks
def _noise_view(noise, row_shape, slots=None):
    """The noise view of a step update: on the device, fp32, [steps, *row_shape] (slots None) or [steps, slots, *row_shape], each row
    contiguous and the rows (and slots) not overlapping - a batch slice of a larger buffer is fine.  Returns the pointer and
    the strides to pass on: (ptr, step stride) or (ptr, step stride, slot stride)."""
    if not noise.is_cuda:
        raise RuntimeError("afldm_amd: noise must live on an MI355X (cuda) device; there is no CPU path")
    lead, n = (() if slots is None else (slots,)), math.prod(row_shape)
    assert noise.dtype == torch.float32 and noise.dim() == 1 + len(lead) + len(row_shape)
    assert tuple(noise.shape[1:]) == lead + tuple(row_shape)
    assert noise[(0,) * (1 + len(lead))].is_contiguous() and noise.stride(len(lead)) >= n
    if slots is None:
        return ptr(noise), noise.stride(0)
    assert noise.stride(0) >= (slots - 1) * noise.stride(1) + n
    return ptr(noise), noise.stride(0), noise.stride(1)


def _slot_tensors(name, x, noises, coefs, names, contiguous=False):
    """The *_step_flat rule for optional noise slots: a None slot must have a zero coefficient; the others are fp32 device tensors
    shaped like x."""
    for z, c, zname in zip(noises, coefs, names):
        if z is None:
            if c != 0.0:
                raise ValueError(f"{name}: {zname} is None but its coefficient is {c}")
            continue
        _dev(z, zname)
        assert z.dtype == torch.float32 and z.shape == x.shape and (z.is_contiguous() or not contiguous)


# ----------------------------------------------------------------------------- stochastic update (DDIM eta != 0, I2SB bridge)
def sde_step(x, eps_nhwc, noise, coef, step_idx, advance=False, out=None):
    """x NCHW fp32 [B, C, H, W], eps NHWC dtype; noise: fp32 view [steps, B, C, H, W] whose last four dimensions are contiguous
    (a batch slice of a larger buffer is fine: the row stride is noise.stride(0)); coef float[8*nsteps] rows
    (p, q, lo, hi, a, b, d, c) and step_idx int32[1] on device."""
    _dev(x, "x"); _dev(eps_nhwc, "eps")
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_sde_step(ptr(x), ptr(eps_nhwc), *_noise_view(noise, x.shape), ptr(out), ptr(coef), ptr(step_idx),
                             int(advance), B, C, H, W, _code(eps_nhwc), stream_ptr()), "sde_step")
    return out


# ----------------------------------------------------------------------------- RePaint inpainting
def repaint_step(x, eps_nhwc, known, mask, noise, coef, step_idx, advance=False, out=None):
    """x, known NCHW fp32 [B, C, H, W], mask fp32 [B, 1, H, W] (1 = keep), eps NHWC dtype; noise: fp32 view [steps, 3, B, C, H, W]
    (slots z_k, z_u, z_b) whose last four dimensions are contiguous (a batch slice of a larger buffer is fine: the strides are
    noise.stride(0) and noise.stride(1)); coef float[12*nsteps] rows (p, q, lo, hi, a, b, c, k0, k1, u0, u1, 0) and step_idx
    int32[1] on device."""
    _dev(x, "x"); _dev(eps_nhwc, "eps"); _dev(known, "known"); _dev(mask, "mask")
    B, C, H, W = x.shape
    assert x.dtype == known.dtype == mask.dtype == torch.float32 and known.shape == x.shape and tuple(mask.shape) == (B, 1, H, W)
    noise_args = _noise_view(noise, x.shape, 3)
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_repaint_step(ptr(x), ptr(eps_nhwc), ptr(known), ptr(mask), *noise_args, ptr(out), ptr(coef), ptr(step_idx),
                                 int(advance), B, C, H, W, _code(eps_nhwc), stream_ptr()), "repaint_step")
    return out


def repaint_step_flat(x, eps, known, mask, noises, row, out=None):
    """x, eps, known, mask: same-shape contiguous fp32 CUDA tensors (the mask expanded to x's shape); noises = (z_k, z_u, z_b),
    each such a tensor or None where its coefficient (k1, c, u1) is 0; row = the floats (p, q, lo, hi, a, b, c, k0, k1, u0, u1)."""
    _dev(x, "x"); _dev(eps, "eps"); _dev(known, "known"); _dev(mask, "mask")
    assert x.dtype == eps.dtype == known.dtype == mask.dtype == torch.float32
    assert x.shape == eps.shape == known.shape == mask.shape
    row = [float(c) for c in row[:11]]
    _slot_tensors("repaint_step_flat", x, noises, (row[8], row[6], row[10]), ("z_k", "z_u", "z_b"))
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_repaint_step_flat(ptr(x), ptr(eps), ptr(known), ptr(mask), *[ptr(z) for z in noises], ptr(out), *row,
                                      x.numel(), stream_ptr()), "repaint_step_flat")
    return out


MASK_MIN, MASK_MEAN = _lib.ABI.constants["AFLDM_MASK_MIN"], _lib.ABI.constants["AFLDM_MASK_MEAN"]


def mask_pool(mask, r, mode=MASK_MIN, out=None):
    """mask fp32 [B, 1, H, W] -> [B, 1, H / r, W / r] over r x r blocks: MASK_MIN (a latent is kept only if every pixel under it is
    kept) or MASK_MEAN.  r >= 1 must divide H and W."""
    _dev(mask, "mask")
    if mask.dtype != torch.float32 or mask.dim() != 4 or mask.shape[1] != 1:
        raise ValueError(f"mask_pool: mask must be fp32 [B, 1, H, W], got {mask.dtype} {tuple(mask.shape)}")
    B, _, H, W = mask.shape
    r = int(r)
    if r < 1 or H % r or W % r:
        raise ValueError(f"mask_pool: r = {r} must be >= 1 and divide H = {H} and W = {W}")
    if out is None:
        out = torch.empty(B, 1, H // r, W // r, dtype=torch.float32, device=mask.device)
    check(lib.afldm_mask_pool(ptr(mask), ptr(out), B, H, W, r, int(mode), stream_ptr()), "mask_pool")
    return out


# ----------------------------------------------------------------------------- image-to-image (SDEdit with a change map)
def sdedit_step(x, eps_nhwc, orig, cmap, z, noise, coef, step_idx, advance=False, out=None):
    """x, orig, z NCHW fp32 [B, C, H, W] (z: the run's one fixed noise), cmap fp32 [B, 1, H, W] (the change map: an element is held
    on orig's noised trajectory while cmap <= the row's thr), eps NHWC dtype; noise: None (no row has c != 0) or an fp32 view
    [steps, B, C, H, W] whose last four dimensions are contiguous (a batch slice of a larger buffer is fine: the row stride is
    noise.stride(0)); coef float[12*nsteps] rows (p, q, lo, hi, a, b, c, k0, k1, thr, 0, 0) and step_idx int32[1] on device."""
    _dev(x, "x"); _dev(eps_nhwc, "eps"); _dev(orig, "orig"); _dev(cmap, "cmap"); _dev(z, "z")
    if x.dim() != 4:
        raise ValueError(f"sdedit_step: x {tuple(x.shape)}, want [B, C, H, W]")
    B, C, H, W = x.shape
    assert x.dtype == orig.dtype == cmap.dtype == z.dtype == torch.float32
    if orig.shape != x.shape or z.shape != x.shape or tuple(cmap.shape) != (B, 1, H, W) or tuple(eps_nhwc.shape) != (B, H, W, C):
        raise ValueError(f"sdedit_step: x {tuple(x.shape)}, orig {tuple(orig.shape)}, z {tuple(z.shape)}, cmap {tuple(cmap.shape)} "
                         f"(want {(B, 1, H, W)}: expand a batch-1 map first), eps {tuple(eps_nhwc.shape)} (want NHWC {(B, H, W, C)})")
    assert x.is_contiguous() and orig.is_contiguous() and cmap.is_contiguous() and z.is_contiguous() and eps_nhwc.is_contiguous()
    noise_args = (None, 0) if noise is None else _noise_view(noise, x.shape)
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_sdedit_step(ptr(x), ptr(eps_nhwc), ptr(orig), ptr(cmap), ptr(z), *noise_args, ptr(out), ptr(coef), ptr(step_idx),
                                int(advance), B, C, H, W, _code(eps_nhwc), stream_ptr()), "sdedit_step")
    return out


def sdedit_step_flat(x, eps, orig, cmap, z, z_u, row, out=None):
    """x, eps, orig, cmap: same-shape contiguous fp32 CUDA tensors (the change map expanded to x's shape); z, z_u: such a tensor, or
    None where its coefficient (k1, c) is 0; row = the floats (p, q, lo, hi, a, b, c, k0, k1, thr)."""
    _dev(x, "x"); _dev(eps, "eps"); _dev(orig, "orig"); _dev(cmap, "cmap")
    assert x.dtype == eps.dtype == orig.dtype == cmap.dtype == torch.float32
    if not (x.shape == eps.shape == orig.shape == cmap.shape):
        raise ValueError(f"sdedit_step_flat: x {tuple(x.shape)}, eps {tuple(eps.shape)}, orig {tuple(orig.shape)}, cmap "
                         f"{tuple(cmap.shape)} must have one shape (expand the change map first)")
    assert x.is_contiguous() and eps.is_contiguous() and orig.is_contiguous() and cmap.is_contiguous()
    row = [float(c) for c in row[:10]]
    _slot_tensors("sdedit_step_flat", x, (z, z_u), (row[8], row[6]), ("z", "z_u"), contiguous=True)
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_sdedit_step_flat(ptr(x), ptr(eps), ptr(orig), ptr(cmap), ptr(z), ptr(z_u), ptr(out), *row, x.numel(),
                                     stream_ptr()), "sdedit_step_flat")
    return out


# ----------------------------------------------------------------------------- bit-reversible sampler (int64 latents)
def _rev_pair(name, far, near, lat, bad):
    """The checks rev_step and rev_step_flat share: far / near contiguous int64 device tensors of one shape, lat fp32 of that
    shape, bad int32 on the device."""
    _dev(far, "far"); _dev(near, "near"); _dev(lat, "lat"); _dev(bad, "bad")
    if far.dtype != torch.int64 or near.dtype != torch.int64 or far.shape != near.shape:
        raise ValueError(f"{name}: far {far.dtype} {tuple(far.shape)} / near {near.dtype} {tuple(near.shape)}, want two int64 tensors "
                         "of one shape")
    if lat.dtype != torch.float32 or lat.shape != near.shape or bad.dtype != torch.int32 or bad.dim() != 1:
        raise ValueError(f"{name}: lat {lat.dtype} {tuple(lat.shape)} (want fp32 {tuple(near.shape)}), bad {bad.dtype} "
                         f"{tuple(bad.shape)} (want int32 [B])")


def rev_step(far, near, eps_nhwc, bad, coef, step_idx, advance=False, out=None):
    """The reversible update on the pair (far, near), int64 NCHW [B, C, H, W] on the grid 2^-32, rotated IN PLACE: far <- near,
    near <- far + sign q (boot: near + sign q), q the integer the row makes of near and eps (afldm_rev_step in afldm_hip.h).  eps
    NHWC dtype; bad int32 [B], set to 1 for a sample with trouble and never cleared here; coef float[4*nsteps] rows (cx, ce, sign,
    boot) and step_idx int32[1] on device.  Returns `out`, the fp32 view of the new near."""
    if out is None:
        out = torch.empty(near.shape, dtype=torch.float32, device=near.device)
    _rev_pair("rev_step", far, near, out, bad)
    _dev(eps_nhwc, "eps")
    if near.dim() != 4:
        raise ValueError(f"rev_step: near {tuple(near.shape)}, want [B, C, H, W]")
    B, C, H, W = near.shape
    if tuple(eps_nhwc.shape) != (B, H, W, C) or bad.shape[0] != B:
        raise ValueError(f"rev_step: eps {tuple(eps_nhwc.shape)} (want NHWC {(B, H, W, C)}), bad {tuple(bad.shape)} (want [{B}])")
    check(lib.afldm_rev_step(ptr(far), ptr(near), ptr(eps_nhwc), ptr(out), ptr(bad), ptr(coef), ptr(step_idx), int(advance),
                             B, C, H, W, _code(eps_nhwc), stream_ptr()), "rev_step")
    return out


def rev_step_flat(far, near, eps, bad, row, out=None):
    """The same update with the row by value, row = (cx, ce, sign, boot): far, near same-shape contiguous int64 CUDA tensors
    [B, ...] rotated in place, eps fp32 of that shape, bad int32 [B].  far may be `near` itself for a boot row (which does not
    read far).  Returns `out`, the fp32 view of the new near."""
    if out is None:
        out = torch.empty(near.shape, dtype=torch.float32, device=near.device)
    _rev_pair("rev_step_flat", far, near, out, bad)
    _dev(eps, "eps")
    if eps.dtype != torch.float32 or eps.shape != near.shape or near.dim() < 1 or bad.shape[0] != near.shape[0]:
        raise ValueError(f"rev_step_flat: eps {eps.dtype} {tuple(eps.shape)} (want fp32 {tuple(near.shape)}), bad {tuple(bad.shape)} "
                         f"(want [{near.shape[0] if near.dim() else '?'}])")
    cx, ce, sign, boot = float(row[0]), float(row[1]), int(row[2]), int(bool(row[3]))
    if sign not in (1, -1) or float(row[2]) != sign:
        raise ValueError(f"rev_step_flat: sign = {row[2]} (want +1 or -1)")
    n = near.numel()
    check(lib.afldm_rev_step_flat(ptr(far), ptr(near), ptr(eps), ptr(out), ptr(bad), cx, ce, sign, boot, n,
                                  max(n // near.shape[0], 1) if n else 1, stream_ptr()), "rev_step_flat")
    return out


def rev_encode(x, bad, out=None):
    """x fp32 [B, ...] -> int64 rn(x 2^32) (ties to even; the product is exact).  bad int32 [B]: 1 is stored for a sample with a
    non-finite value or one of magnitude >= 2^31 (its integer is 0); never cleared here."""
    _dev(x, "x"); _dev(bad, "bad")
    if x.dtype != torch.float32 or x.dim() < 1 or bad.dtype != torch.int32 or tuple(bad.shape) != (x.shape[0],):
        raise ValueError(f"rev_encode: x {x.dtype} {tuple(x.shape)} (want fp32 [B, ...]), bad {bad.dtype} {tuple(bad.shape)} "
                         "(want int32 [B])")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.int64, device=x.device)
    _dev(out, "out")
    if out.dtype != torch.int64 or out.shape != x.shape:
        raise ValueError(f"rev_encode: out {out.dtype} {tuple(out.shape)}, want int64 {tuple(x.shape)}")
    n = x.numel()
    check(lib.afldm_rev_encode(ptr(x), ptr(out), ptr(bad), n, max(n // x.shape[0], 1) if n else 1, stream_ptr()), "rev_encode")
    return out


# ----------------------------------------------------------------------------- ILVR reference-guided sampling
def _ilvr_plane(name, x, Lh, Lw):
    """The checks ilvr_step and ilvr_step_flat share: fp32 [B, C, H, W] latents, Lh fp32 [H, H] and Lw fp32 [W, W] on the device.
    Which planes there is a kernel for (square, 2 .. 64) is the library's to say: it refuses the others before any launch."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"{name}: x must be fp32 [B, C, H, W], got {x.dtype} {tuple(x.shape)}")
    for n, m, s in (("Lh", Lh, x.shape[2]), ("Lw", Lw, x.shape[3])):
        _dev(m, n)
        if m.dtype != torch.float32 or tuple(m.shape) != (s, s):
            raise ValueError(f"{name}: {n} must be an fp32 [{s}, {s}] matrix, got {m.dtype} {tuple(m.shape)}")


def ilvr_step(x, eps_nhwc, ref, noise, Lh, Lw, coef, step_idx, advance=False, out=None):
    """x, ref NCHW fp32 [B, C, S, S], eps NHWC dtype, Lh / Lw fp32 [S, S] (phi(d) = Lh d Lw^T; may be the same tensor); noise:
    fp32 view [steps, 2, B, C, S, S] (slots z_k, z_u) whose last four dimensions are contiguous (a batch slice of a larger buffer
    is fine: the strides are noise.stride(0) and noise.stride(1)); coef float[12*nsteps] rows (p, q, lo, hi, a, b, c, k0, k1, w,
    0, 0) and step_idx int32[1] on device."""
    _dev(x, "x"); _dev(eps_nhwc, "eps"); _dev(ref, "ref")
    _ilvr_plane("ilvr_step", x, Lh, Lw)
    B, C, H, W = x.shape
    assert ref.dtype == torch.float32 and ref.shape == x.shape and x.is_contiguous() and ref.is_contiguous()
    assert tuple(eps_nhwc.shape) == (B, H, W, C) and eps_nhwc.is_contiguous()
    noise_args = _noise_view(noise, x.shape, 2)
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_ilvr_step(ptr(x), ptr(eps_nhwc), ptr(ref), *noise_args, ptr(Lh), ptr(Lw),
                              ptr(out), ptr(coef), ptr(step_idx), int(advance), B, C, H, W, _code(eps_nhwc), stream_ptr()),
          "ilvr_step")
    return out


def ilvr_step_flat(x, eps, ref, noises, Lh, Lw, row, out=None):
    """x, eps, ref: same-shape contiguous fp32 CUDA tensors [B, C, S, S]; noises = (z_k, z_u), each such a tensor or None where it
    is not read (z_k: k1 = 0 or w = 0; z_u: c = 0); Lh / Lw fp32 [S, S]; row = the floats (p, q, lo, hi, a, b, c, k0, k1, w)."""
    _dev(x, "x"); _dev(eps, "eps"); _dev(ref, "ref")
    _ilvr_plane("ilvr_step_flat", x, Lh, Lw)
    assert eps.dtype == ref.dtype == torch.float32 and x.shape == eps.shape == ref.shape
    assert x.is_contiguous() and eps.is_contiguous() and ref.is_contiguous()
    row = [float(c) for c in row[:10]]
    _slot_tensors("ilvr_step_flat", x, noises, (row[8] if row[9] != 0.0 else 0.0, row[6]), ("z_k", "z_u"), contiguous=True)
    if out is None:
        out = torch.empty_like(x)
    B, C, H, W = x.shape
    check(lib.afldm_ilvr_step_flat(ptr(x), ptr(eps), ptr(ref), *[ptr(z) for z in noises], ptr(Lh), ptr(Lw), ptr(out), *row,
                                   B * C, H, W, stream_ptr()), "ilvr_step_flat")
    return out


# ----------------------------------------------------------------------------- perturbed-attention guidance
# fewest tokens per sample the one-launch identity block is used for.  Measured at 32 samples, bf16, captured and replayed,
# alternated rounds (tools/bench_pag.py kernels), one launch against gn_apply + conv2d: T = 1024, C = 192:
# 20.9 against 28.2 us; T = 256, C = 384: 25.0 / 20.9; T = 64, C = 384: 21.4 / 13.1; T = 16, C = 768: 49.3 / 15.6; T = 4, C = 768:
# 56.7 / 11.2 - below the 32^2 level a handful of workgroups each walk the whole W_vo, and the two launches win.
# AFLDM_IDENTITY_MIN_T=4 sends every level the library has a kernel for to the one launch (tests, A/B).
_IDENTITY_MIN_T = int(os.environ.get("AFLDM_IDENTITY_MIN_T", "1024"))


def attn_identity_block_ok(x, G):
    """True when afldm_attn_identity_block has a kernel for tokens x [B, T, C] with G groups (bf16; the shapes: afldm_hip.h) and the
    policy wants it (_IDENTITY_MIN_T)."""
    B, T, C = x.shape
    if x.dtype not in DTYPE_CODE or T < _IDENTITY_MIN_T:
        return False
    return bool(lib.afldm_attn_identity_block_ok(B, T, C, int(G), _code(x)))


def attn_identity_block(x, stats, gamma, beta, G, eps, w_vo, b_vo, out=None):
    """The attention block with its attention map replaced by the identity: y = x + GN(x) W_vo^T + b_vo on tokens x [B, T, C]
    (or NHWC [B, H, W, C]); stats = GNStats of x, w_vo the packed folded weight (blocks.packed_vo), b_vo fp32 [C].  One launch
    where attn_identity_block_ok says so; elsewhere (fp32, other shapes) the two existing launches on the same folded weight,
    gn_apply + conv2d(residual=x).  `out`: a contiguous tensor of x's shape (a batch slice of a larger buffer), not x itself."""
    _dev(x, "x")
    assert x.is_contiguous() and stats.st2 is None and stats.st1.shape[2] == x.shape[-1]
    C = x.shape[-1]
    tokens = x.reshape(x.shape[0], -1, C)
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous() and out.data_ptr() != x.data_ptr()
    if not attn_identity_block_ok(tokens, G):
        hn = gn_apply(x, stats, gamma, beta, G, eps, act=0)
        conv2d(hn, w_vo, b_vo, residual=x, out=out)
        return out
    B, T, _ = tokens.shape
    tok = _begin()
    check(lib.afldm_attn_identity_block(ptr(x), ptr(stats.st1), stats.S1, ptr(gamma), ptr(beta), int(G), float(eps), ptr(w_vo),
                                        ptr(b_vo), ptr(out), B, T, C, _code(x), stream_ptr()), "attn_identity_block")
    _end(tok, "attn_identity", 2.0 * B * T * C * C, (2 * B * T * C + C * C) * x.element_size())
    return out


def _pag_args(name, x, eps2):
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be contiguous fp32 [B, C, H, W], got {x.dtype} {tuple(x.shape)}")
    B, C, H, W = x.shape
    return B, C, H, W


def pag_step(x, eps2_nhwc, noise, coef, step_idx, advance=False, out=None):
    """x NCHW fp32 [B, C, H, W]; eps2 NHWC dtype [2B, H, W, C]: rows 0 .. B-1 the UNet's output, rows B .. 2B-1 the perturbed
    UNet's; noise: None (no row has c != 0) or an fp32 view [steps, B, C, H, W] whose last four dimensions are contiguous; coef
    float[12*nsteps] rows (p, q, lo, hi, a, b, d, c, s, phi, 0, 0) and step_idx int32[1] on device."""
    _dev(x, "x"); _dev(eps2_nhwc, "eps2")
    B, C, H, W = _pag_args("pag_step", x, eps2_nhwc)
    assert tuple(eps2_nhwc.shape) == (2 * B, H, W, C) and eps2_nhwc.is_contiguous()
    noise_args = (None, 0) if noise is None else _noise_view(noise, x.shape)
    if out is None:
        out = torch.empty_like(x)
    check(lib.afldm_pag_step(ptr(x), ptr(eps2_nhwc), *noise_args, ptr(out), ptr(coef), ptr(step_idx), int(advance),
                             B, C, H, W, _code(eps2_nhwc), stream_ptr()), "pag_step")
    return out


def pag_step_flat(x, e, e_p, z, row, out=None):
    """x, e, e_p: same-shape contiguous fp32 CUDA tensors [B, ...] (a sample = everything behind the first dimension); z such a
    tensor, or None where the row's c is 0; row = the floats (p, q, lo, hi, a, b, d, c, s, phi[, 0, 0])."""
    _dev(x, "x"); _dev(e, "e"); _dev(e_p, "e_p")
    assert x.dtype == e.dtype == e_p.dtype == torch.float32 and x.shape == e.shape == e_p.shape and x.dim() >= 2
    assert x.is_contiguous() and e.is_contiguous() and e_p.is_contiguous()
    row = ([float(c) for c in row] + [0.0, 0.0])[:12]
    _slot_tensors("pag_step_flat", x, (z,), (row[7],), ("z",), contiguous=True)
    if out is None:
        out = torch.empty_like(x)
    B = x.shape[0]
    check(lib.afldm_pag_step_flat(ptr(x), ptr(e), ptr(e_p), ptr(z), ptr(out), *row, B, x.numel() // max(B, 1), stream_ptr()),
          "pag_step_flat")
    return out


# ----------------------------------------------------------------------------- self-attention guidance
def gaussian_taps(kernel_size=9, sigma=1.0):
    """diffusers' gaussian_blur_2d window, w = exp(-0.5 (linspace(-k, k, 2 k + 1) / sigma)^2) normalised, k = (kernel_size - 1) / 2,
    computed in float64 and rounded once to fp32: a tuple of Python floats that are exactly those fp32 values (hashable: it goes
    into an engine's cache key)."""
    n = int(kernel_size)
    if n < 1 or n > 15 or n % 2 == 0 or not float(sigma) > 0.0:
        raise ValueError(f"gaussian_taps: kernel_size = {kernel_size} must be odd, 1 .. 15, and sigma = {sigma} positive")
    k = (n - 1) * 0.5
    w = torch.exp(-0.5 * (torch.linspace(-k, k, n, dtype=torch.float64) / float(sigma)) ** 2)
    return tuple(float(v) for v in (w / w.sum()).float())


def attn_key_mass_ok(q, heads):
    """True when afldm_attn_key_mass has a kernel for q [B, T, heads * d] (the shapes: afldm_hip.h)."""
    B, T, C = q.shape
    return q.dtype in DTYPE_CODE and C % heads == 0 and bool(lib.afldm_attn_key_mass_ok(B, int(heads), T, C // heads, _code(q)))


def attn_key_mass(q, k, heads, scale=None, out=None):
    """The attention mass every key receives, mass[b, j] = (1 / heads) sum_h sum_i softmax_j(scale q_bhi . k_bhj), fp32 [B, T]: q, k
    [B, T, C] token-major as ops.attention takes them (column slices of a wider buffer are fine: the leading dimension is
    stride(1)), self-attention only.  The T x T probabilities never reach memory.  A shape without a kernel is an error."""
    if not (q.is_cuda and k.is_cuda):
        raise RuntimeError("afldm_amd: attn_key_mass inputs must live on an MI355X (cuda) device; there is no CPU path")
    B, T, C = q.shape
    assert k.shape == q.shape and k.dtype == q.dtype, "attn_key_mass: self-attention (k shaped like q)"
    ldq, ldk = q.stride(1), k.stride(1)
    assert q.stride(2) == 1 and k.stride(2) == 1 and q.stride(0) == T * ldq and k.stride(0) == T * ldk
    d = C // heads
    if scale is None:
        scale = d ** -0.5
    if out is None:
        out = torch.empty((B, T), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, T) and out.is_contiguous() and out.is_cuda
    ws = torch.empty((B * heads * T * 2,), dtype=torch.float32, device=q.device)
    tok = _begin()
    check(lib.afldm_attn_key_mass(ptr(q), ldq, ptr(k), ldk, ptr(out), ptr(ws), B, int(heads), T, d, float(scale), _code(q),
                                  stream_ptr()), "attn_key_mass")
    _end(tok, "attn_key_mass", 6.0 * B * heads * T * T * d, (4 * B * T * C) * q.element_size())
    return out


def _sag_args(name, x, mass, taps, boundary):
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be contiguous fp32 [B, C, H, W], got {x.dtype} {tuple(x.shape)}")
    B, C, H, W = x.shape
    _dev(mass, "mass")
    if mass.dtype != torch.float32 or mass.dim() != 2 or mass.shape[0] != B or not mass.is_contiguous():
        raise ValueError(f"{name}: mass must be contiguous fp32 [{B}, hm * hm], got {mass.dtype} {tuple(mass.shape)}")
    hm = int(round(mass.shape[1] ** 0.5))
    if hm * hm != mass.shape[1]:
        raise ValueError(f"{name}: {mass.shape[1]} masses per sample are no square map")
    if boundary not in ("reflect", "circular"):
        raise ValueError(f"{name}: boundary {boundary!r} (want 'reflect' or 'circular')")
    w = (ctypes.c_float * len(taps))(*[float(t) for t in taps])
    return B, C, H, W, hm, w, len(taps), int(boundary == "circular")


def sag_degrade(x, e_nhwc, mass, taps, boundary, coef, step_idx, out=None):
    """SAG's degraded UNet input in one launch (afldm_sag_degrade): x NCHW fp32 [B, C, H, W], e NHWC dtype [B, H, W, C] (the UNet's
    output), mass fp32 [B, hm * hm] (attn_key_mass of the chosen site), taps a sequence of fp32-exact floats (gaussian_taps),
    boundary 'reflect' | 'circular'; (p, q) = the first two fields of the 12-float row of `coef` at *step_idx.  Returns x_d NHWC
    in e's dtype: x + M (G x0 - x0) / p with x0 = p x + q e and M = mass > 1 up-sampled to the latent grid."""
    _dev(x, "x"); _dev(e_nhwc, "e")
    B, C, H, W, hm, w, n, bnd = _sag_args("sag_degrade", x, mass, taps, boundary)
    assert tuple(e_nhwc.shape) == (B, H, W, C) and e_nhwc.is_contiguous()
    if out is None:
        out = torch.empty_like(e_nhwc)
    assert out.shape == e_nhwc.shape and out.dtype == e_nhwc.dtype and out.is_contiguous() and out.data_ptr() != e_nhwc.data_ptr()
    check(lib.afldm_sag_degrade(ptr(x), ptr(e_nhwc), ptr(mass), ptr(out), ptr(coef), ptr(step_idx), w, n, bnd, B, C, H, W, hm,
                                _code(e_nhwc), stream_ptr()), "sag_degrade")
    return out


def sag_degrade_flat(x, e, mass, taps, boundary, p, q, out=None):
    """The same on NCHW fp32 tensors throughout with p and q by value (the eager loop): x, e [B, C, H, W] -> x_d [B, C, H, W]."""
    _dev(x, "x"); _dev(e, "e")
    B, C, H, W, hm, w, n, bnd = _sag_args("sag_degrade_flat", x, mass, taps, boundary)
    assert e.shape == x.shape and e.dtype == torch.float32 and e.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous()
    check(lib.afldm_sag_degrade_flat(ptr(x), ptr(e), ptr(mass), ptr(out), float(p), float(q), w, n, bnd, B, C, H, W, hm,
                                     stream_ptr()), "sag_degrade_flat")
    return out


# ----------------------------------------------------------------------------- MultiDiffusion: a canvas through windows
def _geom_args(g):
    """A panorama.Geometry as the C arguments (Hc, Wc, S, oy, ny, ox, nx, wrap_y, wrap_x); the origin lists are host arrays the
    library reads during the call (the kernels get them by value)."""
    oy, ox = (ctypes.c_int * len(g.oy))(*g.oy), (ctypes.c_int * len(g.ox))(*g.ox)
    return g.Hc, g.Wc, g.S, oy, len(g.oy), ox, len(g.ox), int(g.wrap_y), int(g.wrap_x)


def _pano_canvas(name, canvas, g):
    _dev(canvas, "canvas")
    if canvas.dim() != 4 or canvas.dtype != torch.float32 or tuple(canvas.shape[2:]) != (g.Hc, g.Wc):
        raise ValueError(f"{name}: the canvas must be fp32 [P, C, {g.Hc}, {g.Wc}], got {canvas.dtype} {tuple(canvas.shape)}")
    return canvas.shape[0], canvas.shape[1]


def _pano_weights(name, wt, g):
    _dev(wt, "wt")
    if wt.dtype != torch.float32 or tuple(wt.shape) != (g.S, g.S):
        raise ValueError(f"{name}: wt must be an fp32 [{g.S}, {g.S}] plane, got {wt.dtype} {tuple(wt.shape)}")


def pano_step(canvas, eps_nhwc, noise, wt, geometry, coef, step_idx, advance=False, out=None, windows_out=None):
    """The fused MultiDiffusion update (afldm_pano_step): canvas fp32 [P, C, Hc, Wc], eps NHWC dtype [P * nwin, S, S, C] (the UNet's
    output on the windows of `geometry`, a panorama.Geometry), wt fp32 [S, S] > 0, noise: fp32 view [steps, P, C, Hc, Wc] whose
    last four dimensions are contiguous, or None when no row has c != 0; coef float[8*nsteps] "sde" rows and step_idx int32[1] on
    device.  Returns (canvas_out, windows_out): the new canvas (out= may be the canvas itself) and its crops, NCHW fp32
    [P * nwin, C, S, S] - the next UNet input."""
    g = geometry
    P, C = _pano_canvas("pano_step", canvas, g)
    _dev(eps_nhwc, "eps"); _pano_weights("pano_step", wt, g)
    if tuple(eps_nhwc.shape) != (P * g.nwin, g.S, g.S, C):
        raise ValueError(f"pano_step: eps {tuple(eps_nhwc.shape)}, want NHWC {(P * g.nwin, g.S, g.S, C)}")
    noise_args = (None, 0) if noise is None else _noise_view(noise, canvas.shape)
    if out is None:
        out = torch.empty_like(canvas)
    if windows_out is None:
        windows_out = torch.empty(P * g.nwin, C, g.S, g.S, dtype=torch.float32, device=canvas.device)
    _dev(out, "out"); _dev(windows_out, "windows_out")
    assert out.dtype == windows_out.dtype == torch.float32 and out.shape == canvas.shape
    assert tuple(windows_out.shape) == (P * g.nwin, C, g.S, g.S)
    check(lib.afldm_pano_step(ptr(canvas), ptr(eps_nhwc), *noise_args, ptr(wt), ptr(out), ptr(windows_out), ptr(coef),
                              ptr(step_idx), int(advance), P, C, *_geom_args(g), _code(eps_nhwc), stream_ptr()), "pano_step")
    return out, windows_out


def pano_repaint_step(canvas, eps_nhwc, known, mask, noise, wt, geometry, coef, step_idx, advance=False, out=None, windows_out=None):
    """The fused outpainting update (afldm_pano_repaint_step): RePaint on a MultiDiffusion canvas.  canvas, known fp32
    [P, C, Hc, Wc], mask fp32 [P, 1, Hc, Wc] (1 = keep), eps and wt as pano_step; noise: fp32 view [steps, 3, P, C, Hc, Wc] (slots
    z_k, z_u, z_b) whose last four dimensions are contiguous; coef float[12*nsteps] "repaint" rows and step_idx int32[1] on device.
    Returns (canvas_out, windows_out) as pano_step."""
    g = geometry
    P, C = _pano_canvas("pano_repaint_step", canvas, g)
    _dev(eps_nhwc, "eps"); _dev(known, "known"); _dev(mask, "mask"); _pano_weights("pano_repaint_step", wt, g)
    if tuple(eps_nhwc.shape) != (P * g.nwin, g.S, g.S, C):
        raise ValueError(f"pano_repaint_step: eps {tuple(eps_nhwc.shape)}, want NHWC {(P * g.nwin, g.S, g.S, C)}")
    if known.dtype != torch.float32 or known.shape != canvas.shape or not known.is_contiguous():
        raise ValueError(f"pano_repaint_step: known must be contiguous fp32 {tuple(canvas.shape)}, got {known.dtype} "
                         f"{tuple(known.shape)}")
    if mask.dtype != torch.float32 or tuple(mask.shape) != (P, 1, g.Hc, g.Wc) or not mask.is_contiguous():
        raise ValueError(f"pano_repaint_step: mask must be contiguous fp32 {(P, 1, g.Hc, g.Wc)}, got {mask.dtype} "
                         f"{tuple(mask.shape)}")
    noise_args = _noise_view(noise, canvas.shape, 3)
    if out is None:
        out = torch.empty_like(canvas)
    if windows_out is None:
        windows_out = torch.empty(P * g.nwin, C, g.S, g.S, dtype=torch.float32, device=canvas.device)
    _dev(out, "out"); _dev(windows_out, "windows_out")
    assert out.dtype == windows_out.dtype == torch.float32 and out.shape == canvas.shape
    assert tuple(windows_out.shape) == (P * g.nwin, C, g.S, g.S)
    check(lib.afldm_pano_repaint_step(ptr(canvas), ptr(eps_nhwc), ptr(known), ptr(mask), *noise_args, ptr(wt), ptr(out),
                                      ptr(windows_out), ptr(coef), ptr(step_idx), int(advance), P, C, *_geom_args(g),
                                      _code(eps_nhwc), stream_ptr()), "pano_repaint_step")
    return out, windows_out


# ----------------------------------------------------------------------------- high-resolution sampling: local + dilated windows
def _hires_args(name, canvas, g, scale, Lh, Lw):
    """The checks hires_step and hires_windows share: (P, C, windows per canvas, the C geometry arguments)."""
    P, C = _pano_canvas(name, canvas, g)
    if g.wrap_y or g.wrap_x:
        raise ValueError(f"{name}: the canvas does not wrap")
    if not canvas.is_contiguous():
        raise ValueError(f"{name}: the canvas must be contiguous")
    for m, n in ((Lh, "Lh"), (Lw, "Lw")):
        if m is None:
            continue
        _dev(m, n)
        if m.dtype != torch.float32 or tuple(m.shape) != (g.Hc, g.Wc) or not m.is_contiguous():
            raise ValueError(f"{name}: {n} must be a contiguous fp32 [{g.Hc}, {g.Wc}] matrix, got {m.dtype} {tuple(m.shape)}")
    return P, C, g.nwin + int(scale) ** 2, _geom_args(g)[:7] + (int(scale),)


def hires_step(canvas, eps_nhwc, ref, eps_ref, noise, wt, Lh, Lw, geometry, scale, coef, step_idx, advance=False, out=None,
               windows_out=None):
    """The fused high-resolution update (afldm_hires_step): canvas, ref, eps_ref fp32 [P, C, Hc, Hc] with Hc = scale * S; eps NHWC
    dtype [P * NW, S, S, C], NW = nwin + scale^2 - the UNet's output on the local windows of `geometry` (a panorama.Geometry, no
    wrap) followed by the scale^2 dilated windows of each canvas; wt fp32 [S, S] > 0; Lh, Lw fp32 [Hc, Hc]; noise: fp32 view
    [steps, P, C, Hc, Hc] whose last four dimensions are contiguous, or None when no row has c != 0; coef float[12*nsteps]
    "hires" rows and step_idx int32[1] on device.  Returns (canvas_out, windows_out): the new canvas (out= may be the canvas
    itself) and the next UNet input, NCHW fp32 [P * NW, C, S, S]."""
    g = geometry
    P, C, NW, geom = _hires_args("hires_step", canvas, g, scale, Lh, Lw)
    _dev(eps_nhwc, "eps"); _dev(ref, "ref"); _dev(eps_ref, "eps_ref"); _pano_weights("hires_step", wt, g)
    if tuple(eps_nhwc.shape) != (P * NW, g.S, g.S, C) or not eps_nhwc.is_contiguous():
        raise ValueError(f"hires_step: eps {tuple(eps_nhwc.shape)}, want contiguous NHWC {(P * NW, g.S, g.S, C)}")
    for t, n in ((ref, "ref"), (eps_ref, "eps_ref")):
        if t.dtype != torch.float32 or t.shape != canvas.shape or not t.is_contiguous():
            raise ValueError(f"hires_step: {n} must be contiguous fp32 {tuple(canvas.shape)}, got {t.dtype} {tuple(t.shape)}")
    noise_args = (None, 0) if noise is None else _noise_view(noise, canvas.shape)
    if out is None:
        out = torch.empty_like(canvas)
    if windows_out is None:
        windows_out = torch.empty(P * NW, C, g.S, g.S, dtype=torch.float32, device=canvas.device)
    _dev(out, "out"); _dev(windows_out, "windows_out")
    assert out.dtype == windows_out.dtype == torch.float32 and out.shape == canvas.shape and out.is_contiguous()
    assert tuple(windows_out.shape) == (P * NW, C, g.S, g.S) and windows_out.is_contiguous()
    check(lib.afldm_hires_step(ptr(canvas), ptr(eps_nhwc), ptr(ref), ptr(eps_ref), *noise_args, ptr(wt), ptr(Lh), ptr(Lw), ptr(out),
                               ptr(windows_out), ptr(coef), ptr(step_idx), int(advance), P, C, *geom, _code(eps_nhwc), stream_ptr()),
          "hires_step")
    return out, windows_out


def hires_windows(canvas, Lh, Lw, f, geometry, scale, out=None):
    """canvas fp32 [P, C, Hc, Hc] -> the UNet input of a high-resolution evaluation, NCHW fp32 [P * NW, C, S, S]: the local crops
    and the dilated views of canvas + f (Lh canvas Lw^T - canvas) (afldm_hires_windows: the tail of hires_step, the same bits).
    Lh / Lw may be None when f == 0."""
    g = geometry
    P, C, NW, geom = _hires_args("hires_windows", canvas, g, scale, Lh, Lw)
    if out is None:
        out = torch.empty(P * NW, C, g.S, g.S, dtype=torch.float32, device=canvas.device)
    _dev(out, "out")
    assert out.dtype == torch.float32 and tuple(out.shape) == (P * NW, C, g.S, g.S) and out.is_contiguous()
    check(lib.afldm_hires_windows(ptr(canvas), ptr(Lh), ptr(Lw), float(f), ptr(out), P, C, *geom, stream_ptr()), "hires_windows")
    return out


def window_fuse(windows, wt, geometry, out=None):
    """windows NCHW fp32 / bf16 [P * nwin, C, S, S] -> the fp32 canvas [P, C, Hc, Wc] of their wt-weighted mean over the windows
    that cover each element (afldm_window_fuse); wt fp32 [S, S] > 0."""
    g = geometry
    _dev(windows, "windows"); _pano_weights("window_fuse", wt, g)
    if windows.dim() != 4 or windows.shape[0] % g.nwin or tuple(windows.shape[2:]) != (g.S, g.S):
        raise ValueError(f"window_fuse: windows {tuple(windows.shape)}, want [P * {g.nwin}, C, {g.S}, {g.S}]")
    P, C = windows.shape[0] // g.nwin, windows.shape[1]
    if out is None:
        out = torch.empty(P, C, g.Hc, g.Wc, dtype=torch.float32, device=windows.device)
    assert (P, C) == _pano_canvas("window_fuse", out, g)
    check(lib.afldm_window_fuse(ptr(windows), ptr(wt), ptr(out), P, C, *_geom_args(g), _code(windows), stream_ptr()), "window_fuse")
    return out


def window_crop(canvas, geometry, out=None):
    """canvas fp32 [P, C, Hc, Wc] -> its windows NCHW fp32 [P * nwin, C, S, S], window k = iy * nx + ix of canvas P at batch entry
    P * nwin + k, with wrap on the circular axes (afldm_window_crop).  Exact."""
    g = geometry
    P, C = _pano_canvas("window_crop", canvas, g)
    if out is None:
        out = torch.empty(P * g.nwin, C, g.S, g.S, dtype=torch.float32, device=canvas.device)
    _dev(out, "out")
    assert out.dtype == torch.float32 and tuple(out.shape) == (P * g.nwin, C, g.S, g.S)
    check(lib.afldm_window_crop(ptr(canvas), ptr(out), P, C, *_geom_args(g), stream_ptr()), "window_crop")
    return out


def select_timestep(tvals, step_idx, t_out, pre_advance=False):
    check(lib.afldm_select_timestep(ptr(tvals), ptr(step_idx), ptr(t_out), int(pre_advance), stream_ptr()),
          "select_timestep")
    return t_out


def select_step_row(tvals, step_idx, t_out, table, row_out, pre_advance=False):
    """afldm_select_step_row: select_timestep + row_out <- table[step] in one launch."""
    assert table.is_contiguous() and row_out.is_contiguous() and table[0].numel() == row_out.numel()
    nbytes = row_out.numel() * row_out.element_size()
    check(lib.afldm_select_step_row(ptr(tvals), ptr(step_idx), ptr(t_out), int(pre_advance), ptr(table), ptr(row_out),
                                    nbytes, stream_ptr()), "select_step_row")
    return t_out


# ----------------------------------------------------------------------------- class conditioning (classifier-free guidance)
def _cond_rows(name, class_rows, out):
    _dev(class_rows, "class_rows")
    if class_rows.dim() != 2 or class_rows.dtype not in DTYPE_CODE:
        raise ValueError(f"{name}: class_rows must be [rows, D] in fp32 or bf16, got {class_rows.dtype} {tuple(class_rows.shape)}")
    if out is None:
        out = torch.empty_like(class_rows)
    _dev(out, "out")
    assert out.shape == class_rows.shape and out.dtype == class_rows.dtype
    return out


def cond_embed(emb_table, step_idx, class_rows, out=None):
    """afldm_cond_embed: out[r] = silu(rnd(emb_table[*step_idx] + class_rows[r])) - emb_table [n, D] the time embeddings per step
    BEFORE the SiLU, class_rows / out [rows, D], all in one dtype; step_idx int32 [1] on the device, read only.  A counter outside
    [0, n) leaves `out` untouched."""
    out = _cond_rows("cond_embed", class_rows, out)
    _dev(emb_table, "emb_table"); _dev(step_idx, "step_idx")
    assert emb_table.dim() == 2 and emb_table.dtype == class_rows.dtype and emb_table.shape[1] == class_rows.shape[1]
    assert step_idx.dtype == torch.int32 and step_idx.numel() == 1
    rows, D = class_rows.shape
    check(lib.afldm_cond_embed(ptr(emb_table), emb_table.shape[0], ptr(step_idx), ptr(class_rows), ptr(out), rows, D,
                               _code(class_rows), stream_ptr()), "cond_embed")
    return out


def cond_embed_flat(emb, class_rows, out=None):
    """afldm_cond_embed_flat: out[r] = silu(rnd(emb[r or 0] + class_rows[r])) - emb [1 | rows, D] (one row is broadcast)."""
    out = _cond_rows("cond_embed_flat", class_rows, out)
    _dev(emb, "emb")
    assert emb.dim() == 2 and emb.dtype == class_rows.dtype and emb.shape[1] == class_rows.shape[1]
    rows, D = class_rows.shape
    check(lib.afldm_cond_embed_flat(ptr(emb), emb.shape[0], ptr(class_rows), ptr(out), rows, D, _code(class_rows), stream_ptr()),
          "cond_embed_flat")
    return out


# ----------------------------------------------------------------------------- slot sampler (a step counter per batch row)
def _slot_ints(B, **tensors):
    for name, t in tensors.items():
        _dev(t, name)
        assert t.dtype == torch.int32 and t.numel() == B, f"slot sampler: {name} must be int32 [{B}]"


def slot_select(row_t, row_temb, pos, end, t_out, active, temb_table, temb_rows):
    """afldm_slot_select: for every slot b with pos[b] + 1 < end[b]: pos[b] += 1, t_out[b] = row_t[pos[b]], active[b] = 1 and
    temb_rows[b] <- temb_table[row_temb[pos[b]]]; otherwise active[b] = 0 and nothing else.  row_t fp32 [R], row_temb int32 [R],
    pos / end / active int32 [B], t_out fp32 [B], temb_table [T, n], temb_rows [B, n] (rows of whole 16-byte chunks)."""
    B, R, T = pos.numel(), row_t.numel(), temb_table.shape[0]
    _slot_ints(B, pos=pos, end=end, active=active)
    for name, t in (("row_t", row_t), ("row_temb", row_temb), ("t_out", t_out), ("temb_table", temb_table), ("temb_rows", temb_rows)):
        _dev(t, name)
    assert row_t.dtype == t_out.dtype == torch.float32 and row_temb.dtype == torch.int32 and row_temb.numel() == R
    assert t_out.numel() == B and temb_table.dim() == 2 and tuple(temb_rows.shape) == (B, temb_table.shape[1])
    assert temb_table.dtype == temb_rows.dtype
    nbytes = temb_table.shape[1] * temb_table.element_size()
    check(lib.afldm_slot_select(ptr(row_t), ptr(row_temb), ptr(pos), ptr(end), ptr(t_out), ptr(active), ptr(temb_table),
                                ptr(temb_rows), B, R, T, nbytes, stream_ptr()), "slot_select")
    return t_out


def slot_step(x, eps_nhwc, row_coef, pos, active):
    """afldm_slot_step, in place: slot b of x (NCHW fp32) with active[b] != 0 takes ddim_step's update with the row
    row_coef[pos[b]] (row_coef fp32 [R, 4]); the other slots are not touched.  eps NHWC dtype."""
    _dev(x, "x"); _dev(eps_nhwc, "eps"); _dev(row_coef, "row_coef")
    B, C, H, W = x.shape
    _slot_ints(B, pos=pos, active=active)
    assert x.dtype == row_coef.dtype == torch.float32 and row_coef.dim() == 2 and row_coef.shape[1] == 4
    assert tuple(eps_nhwc.shape) == (B, H, W, C)
    check(lib.afldm_slot_step(ptr(x), ptr(eps_nhwc), ptr(row_coef), ptr(pos), ptr(active), B, row_coef.shape[0], C, H, W,
                              _code(eps_nhwc), stream_ptr()), "slot_step")
    return x


def slot_step_kinds(x, eps_nhwc, hist, row_coef, row_kind, pos, active):
    """afldm_slot_step_kinds (include/afldm_hip_slots.h, libafldm_slots.so), in place: slot b of x (NCHW fp32) with active[b] != 0 takes the update of its row's kind
    (row_kind int32 [R]: 0 = ddim_step's with the first four floats of row_coef[pos[b]], 1 = dpm_step's with the row's first six
    and the slot's own planes of hist fp32 [2, B, C, H, W]); row_coef fp32 [R, 8].  The other slots, and a "ddim" slot's history,
    are not touched.  eps NHWC dtype."""
    for name, t in (("x", x), ("eps", eps_nhwc), ("hist", hist), ("row_coef", row_coef), ("row_kind", row_kind)):
        _dev(t, name)
    B, C, H, W = x.shape
    _slot_ints(B, pos=pos, active=active)
    assert x.dtype == hist.dtype == row_coef.dtype == torch.float32 and row_coef.dim() == 2 and row_coef.shape[1] == 8
    assert row_kind.dtype == torch.int32 and row_kind.numel() == row_coef.shape[0]
    assert tuple(eps_nhwc.shape) == (B, H, W, C) and tuple(hist.shape) == (2, B, C, H, W)
    from . import _slots              # (libafldm_slots.so, loaded on first use)
    check(_slots.lib().afldm_slot_step_kinds(ptr(x), ptr(eps_nhwc), ptr(hist), ptr(row_coef), ptr(row_kind), ptr(pos),
                                             ptr(active), B, row_coef.shape[0], C, H, W, _code(eps_nhwc), stream_ptr()),
          "slot_step_kinds")
    return x


# ----------------------------------------------------------------------------- counter-based device noise (libafldm_noise.so)
def _seeds(seeds, B):
    _dev(seeds, "seeds")
    assert seeds.dtype == torch.int64 and seeds.is_contiguous() and seeds.numel() == B, f"seeds: int64 [{B}]"


def philox_bits(seeds, groups, g0=0, ordinal=0, slot=0, c3=0, out=None):
    """afldm_philox_bits (include/afldm_hip_noise.h): int32 [B, groups, 4] holding the raw Philox-4x32-10 words (as bit patterns)
    of the counters (g0 + g, ordinal, slot, c3) - the low 32 bits of each - under the key of seeds[b] (int64 [B] on the device)."""
    B = seeds.numel()
    _seeds(seeds, B)
    if out is None:
        out = torch.empty((B, int(groups), 4), dtype=torch.int32, device=seeds.device)
    assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (B, int(groups), 4)
    from . import _noise              # (libafldm_noise.so, loaded on first use)
    check(_noise.lib().afldm_philox_bits(ptr(out), ptr(seeds), int(g0), int(ordinal), int(slot), int(c3), B, int(groups),
                                         stream_ptr()), "philox_bits")
    return out


def counter_noise(seeds, ordinals, shape, slot=0, out=None):
    """afldm_counter_noise: the counter-based normal stream, fp32 NCHW `shape` = [B, C, H, W]; sample b from seeds[b] (int64 [B]) at
    the step ordinal ordinals[b] (int32 [B]) and noise slot `slot`.  out: a contiguous fp32 tensor (or view) of that shape."""
    B, C, H, W = (int(v) for v in shape)
    _seeds(seeds, B)
    _slot_ints(B, ordinals=ordinals)
    if out is None:
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=seeds.device)
    _dev(out, "out")
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, C, H, W)
    from . import _noise
    check(_noise.lib().afldm_counter_noise(ptr(out), ptr(seeds), ptr(ordinals), int(slot), B, C, H, W, stream_ptr()),
          "counter_noise")
    return out


def seeded_step(x, eps_nhwc, seeds, coef, step_idx, advance=False, out=None):
    """afldm_seeded_step: sde_step with the noise made in registers - sample b's from seeds[b] (int64 [B]) at the ordinal
    *step_idx, noise slot 0.  x NCHW fp32 [B, C, H, W], eps NHWC dtype; coef float[8*nsteps] rows (p, q, lo, hi, a, b, d, c) and
    step_idx int32[1] on device."""
    _dev(x, "x"); _dev(eps_nhwc, "eps"); _dev(coef, "coef")
    B, C, H, W = x.shape
    _seeds(seeds, B)
    assert x.dtype == torch.float32 and tuple(eps_nhwc.shape) == (B, H, W, C)
    if out is None:
        out = torch.empty_like(x)
    from . import _noise
    check(_noise.lib().afldm_seeded_step(ptr(x), ptr(eps_nhwc), ptr(seeds), ptr(out), ptr(coef), ptr(step_idx), int(advance),
                                         B, C, H, W, _code(eps_nhwc), stream_ptr()), "seeded_step")
    return out


def slot_step_seeded(x, eps_nhwc, hist, row_coef, row_kind, row_ord, pos, active, seeds):
    """afldm_slot_step_seeded, in place: slot_step_kinds plus kind code 2 - seeded_step's update with the row row_coef[pos[b]], the
    ordinal row_ord[pos[b]] (int32 [R]) and the seed seeds[b] (int64 [B]); such a slot's history planes are not touched."""
    for name, t in (("x", x), ("eps", eps_nhwc), ("hist", hist), ("row_coef", row_coef), ("row_kind", row_kind), ("row_ord", row_ord)):
        _dev(t, name)
    B, C, H, W = x.shape
    _slot_ints(B, pos=pos, active=active)
    _seeds(seeds, B)
    assert x.dtype == hist.dtype == row_coef.dtype == torch.float32 and row_coef.dim() == 2 and row_coef.shape[1] == 8
    assert row_kind.dtype == row_ord.dtype == torch.int32 and row_kind.numel() == row_ord.numel() == row_coef.shape[0]
    assert tuple(eps_nhwc.shape) == (B, H, W, C) and tuple(hist.shape) == (2, B, C, H, W)
    from . import _noise
    check(_noise.lib().afldm_slot_step_seeded(ptr(x), ptr(eps_nhwc), ptr(hist), ptr(row_coef), ptr(row_kind), ptr(row_ord),
                                              ptr(pos), ptr(active), ptr(seeds), B, row_coef.shape[0], C, H, W, _code(eps_nhwc),
                                              stream_ptr()), "slot_step_seeded")
    return x


def slot_step_edit(x, eps_nhwc, hist, cond, cmask, row_coef, row_kind, row_ord, pos, active, seeds):
    """afldm_slot_step_edit (include/afldm_hip_edit.h, libafldm_edit.so), in place: slot_step_seeded on 12-wide rows plus the kind
    codes 3 - "seeded_sdedit": img2img's select between the slot's original cond[b], noised by the run's one noise, and the reverse
    step, by its change map cmask[b] - and 4 - "seeded_repaint": RePaint's blend of the slot's known latents cond[b] and the reverse
    step by its mask cmask[b], and the jump.  cond fp32 [B, C, H, W], cmask fp32 [B, 1, H, W]; every noise is the counter stream of
    seeds[b] at the ordinal row_ord[pos[b]].  Such a slot's history planes are not touched."""
    for name, t in (("x", x), ("eps", eps_nhwc), ("hist", hist), ("cond", cond), ("cmask", cmask), ("row_coef", row_coef),
                    ("row_kind", row_kind), ("row_ord", row_ord)):
        _dev(t, name)
    B, C, H, W = x.shape
    _slot_ints(B, pos=pos, active=active)
    _seeds(seeds, B)
    assert x.dtype == hist.dtype == cond.dtype == cmask.dtype == row_coef.dtype == torch.float32
    assert row_coef.dim() == 2 and row_coef.shape[1] == 12
    assert row_kind.dtype == row_ord.dtype == torch.int32 and row_kind.numel() == row_ord.numel() == row_coef.shape[0]
    assert tuple(eps_nhwc.shape) == (B, H, W, C) and tuple(hist.shape) == (2, B, C, H, W)
    assert tuple(cond.shape) == (B, C, H, W) and tuple(cmask.shape) == (B, 1, H, W)
    from . import _edit               # (libafldm_edit.so, loaded on first use)
    check(_edit.lib().afldm_slot_step_edit(ptr(x), ptr(eps_nhwc), ptr(hist), ptr(cond), ptr(cmask), ptr(row_coef), ptr(row_kind),
                                           ptr(row_ord), ptr(pos), ptr(active), ptr(seeds), B, row_coef.shape[0], C, H, W,
                                           _code(eps_nhwc), stream_ptr()), "slot_step_edit")
    return x


def slot_exchange(cmd, lat, out, fresh, pos, end):
    """afldm_slot_exchange: cmd int32 [B, 4] = {harvest, refill, begin, end} per slot - out[harvest] <- lat[b] where harvest >= 0,
    then lat[b] <- fresh[refill], pos[b] = begin - 1, end[b] = end where refill >= 0.  lat [B, ...], out [No, ...], fresh
    [Nf, ...] fp32 with equal trailing shapes."""
    B = lat.shape[0]
    for name, t in (("cmd", cmd), ("lat", lat), ("out", out), ("fresh", fresh)):
        _dev(t, name)
    _slot_ints(B, pos=pos, end=end)
    assert cmd.dtype == torch.int32 and tuple(cmd.shape) == (B, 4)
    assert lat.dtype == out.dtype == fresh.dtype == torch.float32 and lat.shape[1:] == out.shape[1:] == fresh.shape[1:]
    check(lib.afldm_slot_exchange(ptr(cmd), ptr(lat), ptr(out), ptr(fresh), ptr(pos), ptr(end), B, lat[0].numel(), out.shape[0],
                                  fresh.shape[0], stream_ptr()), "slot_exchange")
    return lat


# ----------------------------------------------------------------------------- parallel-in-time sampling (Picard sweeps over a window)
def picard_blocks(C, H, W):
    """Blocks of an afldm_picard_sweep per image: the last dimension of its workspace `partial` [P, Wn, blocks]."""
    n = lib.afldm_picard_blocks(int(C), int(H), int(W))
    if n <= 0:
        raise ValueError(f"picard_blocks: bad shape ({C}, {H}, {W})")
    return n


def _picard_states(x, y):
    _dev(x, "x"); _dev(y, "y")
    assert x.dtype == y.dtype == torch.float32 and x.dim() == 5 and x.shape[0] >= 2, "picard: x must be fp32 [Wn + 1, P, C, H, W]"
    Wn, P, C, H, W = x.shape[0] - 1, *x.shape[1:]
    assert tuple(y.shape) == (Wn, P, C, H, W), f"picard: y must be [{Wn}, {P}, {C}, {H}, {W}]"
    return Wn, P, C, H, W


def picard_sweep(x, eps_nhwc, y, partial, row_coef, base):
    """afldm_picard_sweep: x fp32 [Wn + 1, P, C, H, W] (the states X[0 .. Wn] of every image), eps NHWC dtype [Wn P, H, W, C] (row
    j P + p evaluated at X[j] of image p), y fp32 [Wn, P, C, H, W] <- Y[1 .. Wn], partial fp32 [P, Wn, picard_blocks(C, H, W)] <-
    the blocks' sums of (Y[j + 1] - X[j + 1])^2; row_coef fp32 [n, 4], base int32 [P] (read only).  A finished image (base[p] == n)
    is skipped."""
    Wn, P, C, H, W = _picard_states(x, y)
    _dev(eps_nhwc, "eps"); _dev(partial, "partial"); _dev(row_coef, "row_coef")
    _slot_ints(P, base=base)
    assert row_coef.dtype == partial.dtype == torch.float32 and row_coef.dim() == 2 and row_coef.shape[1] == 4
    assert tuple(eps_nhwc.shape) == (Wn * P, H, W, C) and tuple(partial.shape) == (P, Wn, picard_blocks(C, H, W))
    check(lib.afldm_picard_sweep(ptr(x), ptr(eps_nhwc), ptr(y), ptr(partial), ptr(row_coef), ptr(base), P, Wn, row_coef.shape[0],
                                 C, H, W, _code(eps_nhwc), stream_ptr()), "picard_sweep")
    return y


def picard_stride(partial, cur, stride, err, log, row_t, row_temb, t_out, active, temb_table, temb_rows, tol2, shape,
                  gather_only=False):
    """afldm_picard_stride: per image p, err[p, j] = sum_b partial[p, j, b] / (C H W); s = min(first j + 1 with err[p, j] > tol2,
    else Wn; n - base[p]); stride[p] = s; base[p] += s; log[iter[p], p] = s; iter[p] += 1 - cur int32 [2, P] holds (base, iter) -
    then t_out / active / temb_rows [Wn P] are gathered for the rows base[p] + j (slot_select's tables: row_t fp32 [n], row_temb
    int32 [n], temb_table [T, width]).  A finished image: s = 0 and nothing gathered.  shape = (C, H, W) of a state;
    gather_only: no decision, no advance, the gather alone."""
    _dev(partial, "partial"); _dev(cur, "cur"); _dev(err, "err"); _dev(log, "log")
    P, Wn = partial.shape[0], partial.shape[1]
    C, H, W = (int(v) for v in shape)
    n, T = row_t.numel(), temb_table.shape[0]
    _slot_ints(P, stride=stride)
    _slot_ints(Wn * P, active=active)
    for name, t in (("row_t", row_t), ("row_temb", row_temb), ("t_out", t_out), ("temb_table", temb_table), ("temb_rows", temb_rows)):
        _dev(t, name)
    assert partial.dtype == err.dtype == torch.float32 and tuple(partial.shape) == (P, Wn, picard_blocks(C, H, W))
    assert cur.dtype == log.dtype == torch.int32 and tuple(cur.shape) == (2, P) and tuple(err.shape) == (P, Wn)
    assert log.dim() == 2 and log.shape[1] == P
    assert row_t.dtype == t_out.dtype == torch.float32 and row_temb.dtype == torch.int32 and row_temb.numel() == n
    assert t_out.numel() == Wn * P and temb_table.dim() == 2 and tuple(temb_rows.shape) == (Wn * P, temb_table.shape[1])
    assert temb_table.dtype == temb_rows.dtype
    nbytes = temb_table.shape[1] * temb_table.element_size()
    check(lib.afldm_picard_stride(ptr(partial), ptr(cur[0]), ptr(cur[1]), ptr(stride), ptr(err), ptr(log), log.shape[0], ptr(row_t),
                                  ptr(row_temb), ptr(t_out), ptr(active), ptr(temb_table), ptr(temb_rows), float(tol2),
                                  int(bool(gather_only)), P, Wn, n, C, H, W, T, nbytes, stream_ptr()), "picard_stride")
    return stride


def picard_slide(x, y, stride):
    """afldm_picard_slide, in place: X[j] of image p <- Y[min(j + stride[p], Wn)], j = 0 .. Wn (x, y as picard_sweep); an image
    whose stride is 0 is not touched."""
    Wn, P, C, H, W = _picard_states(x, y)
    _slot_ints(P, stride=stride)
    check(lib.afldm_picard_slide(ptr(x), ptr(y), ptr(stride), P, Wn, C, H, W, stream_ptr()), "picard_slide")
    return x


FLOW_PICK, FLOW_POOL = _lib.ABI.constants["AFLDM_FLOW_PICK"], _lib.ABI.constants["AFLDM_FLOW_POOL"]


def flow_splat_workspace(B, C, H, W, ds, mode):
    """fp32 elements of afldm_flow_splat's accumulation workspace."""
    n = lib.afldm_flow_splat_workspace(B, C, H, W, ds, mode)
    if n == 0:
        raise ValueError(f"flow_splat: bad arguments (B {B}, C {C}, H {H}, W {W}, ds {ds}, mode {mode}): H and W must be multiples of ds")
    return n // 4


def flow_splat(x, flow, scale, ds=1, mode=FLOW_PICK, fill=None, fill_pix_stride=1, out=None, occ=None, workspace=None):
    """afldm_flow_splat: forward bilinear splat of x [Bs, C, H, W] along scale[b] * flow [Bs, 2, H, W] (fp32, channel 0 = row
    displacement) for B = scale.numel() samples (sample b reads source b // (B // Bs)), then the finishing pass.
      FLOW_PICK: (res [B, C, H/ds, W/ds], occ [B, 1, H/ds, W/ds]): the warp at every ds-th pixel; fill: [1 | B, C, H/ds * fps,
        W/ds * fps] with fps = fill_pix_stride, applied as res * (1 - occ) + occ * fill[..., ::fps, ::fps].
      FLOW_POOL: (pooled [B, C, H/ds, W/ds], occ [B, 1, H, W]): sum over ds x ds blocks of (fill * occ + res * (1 - occ)) / ds;
        fill: [1 | B, C, H, W] or None (0).
    scale is read when the kernels run (a captured call replays new values).  workspace: fp32 device tensor of at least
    flow_splat_workspace(...) elements (allocated when None); the call zeroes it."""
    _dev(x, "x"); _dev(flow, "flow"); _dev(scale, "scale")
    Bs, C, H, W = x.shape
    B = scale.numel()
    if flow.dtype != torch.float32 or tuple(flow.shape) != (Bs, 2, H, W):
        raise ValueError(f"flow_splat: flow must be fp32 [{Bs}, 2, {H}, {W}], got {flow.dtype} {tuple(flow.shape)}")
    if scale.dtype != torch.float32 or scale.dim() != 1 or B % Bs:
        raise ValueError(f"flow_splat: scale must be fp32 [B] with B a multiple of {Bs}, got {scale.dtype} {tuple(scale.shape)}")
    if mode not in (FLOW_PICK, FLOW_POOL):
        raise ValueError(f"flow_splat: unknown mode {mode!r}")
    nws = flow_splat_workspace(B, C, H, W, ds, mode)
    Ho, Wo = H // ds, W // ds
    fbs = 0
    if fill is not None:
        _dev(fill, "fill")
        fps = 1 if mode == FLOW_POOL else int(fill_pix_stride)
        want = (C, H, W) if mode == FLOW_POOL else (C, Ho * fps, Wo * fps)
        if fill.dtype != x.dtype or fill.dim() != 4 or fill.shape[0] not in (1, B) or tuple(fill.shape[1:]) != want:
            raise ValueError(f"flow_splat: fill must be {x.dtype} [1 or {B}, {want[0]}, {want[1]}, {want[2]}], got {fill.dtype} "
                             f"{tuple(fill.shape)}")
        fbs = 0 if fill.shape[0] == 1 else fill.stride(0)
    if workspace is None:
        workspace = torch.empty(nws, dtype=torch.float32, device=x.device)
    _dev(workspace, "workspace")
    if workspace.dtype != torch.float32 or workspace.numel() < nws:
        raise ValueError(f"flow_splat: workspace must be fp32 with at least {nws} elements")
    occ_shape = (B, 1, H, W) if mode == FLOW_POOL else (B, 1, Ho, Wo)
    if out is None:
        out = torch.empty((B, C, Ho, Wo), dtype=x.dtype, device=x.device)
    if occ is None:
        occ = torch.empty(occ_shape, dtype=x.dtype, device=x.device)
    _dev(out, "out"); _dev(occ, "occ")
    assert tuple(out.shape) == (B, C, Ho, Wo) and tuple(occ.shape) == occ_shape and out.dtype == occ.dtype == x.dtype
    check(lib.afldm_flow_splat(ptr(x), ptr(flow), ptr(scale), ptr(fill), fbs, int(fill_pix_stride), ptr(out), ptr(occ),
                               ptr(workspace), workspace.numel() * 4, B, Bs, C, H, W, int(ds), mode, _code(x), stream_ptr()),
          "flow_splat")
    return out, occ


def flow_warp(x, flow, add_grid=True, nearest=False, mask=False):
    """afldm_flow_warp: grid_sample(align_corners=True, zeros) of x [B, C, Hin, Win] at coords_grid + flip(flow) (add_grid; flow
    fp32 [B, 2, Hout, Wout], channel 0 = row displacement) or at the coordinates `flow` itself holds (channel 0 = x).  Returns
    y [B, C, Hout, Wout], and with mask=True also the reference's in-bounds mask (bool [B, Hout, Wout])."""
    _dev(x, "x"); _dev(flow, "flow")
    B, C, Hi, Wi = x.shape
    if flow.dtype != torch.float32 or flow.dim() != 4 or flow.shape[0] != B or flow.shape[1] != 2:
        raise ValueError(f"flow_warp: flow / coordinates must be fp32 [{B}, 2, H, W], got {flow.dtype} {tuple(flow.shape)}")
    Ho, Wo = flow.shape[-2:]
    y = torch.empty((B, C, Ho, Wo), dtype=x.dtype, device=x.device)
    m = torch.empty((B, Ho, Wo), dtype=torch.bool, device=x.device) if mask else None
    check(lib.afldm_flow_warp(ptr(x), ptr(flow), ptr(y), ptr(m), B, C, Hi, Wi, Ho, Wo, int(bool(add_grid)), int(bool(nearest)),
                              _code(x), stream_ptr()), "flow_warp")
    return (y, m) if mask else y


def _flowest_planes(t, name):
    _dev(t, name)
    if t.dtype != torch.float32 or t.dim() < 2:
        raise ValueError(f"{name} must be fp32 [..., H, W], got {t.dtype} {tuple(t.shape)}")
    H, W = t.shape[-2:]
    return t.numel() // (H * W), H, W


def flowest_pyr_down(x, factor=2, out=None):
    """afldm_flowest_pyr_down: x [..., H, W] (fp32 / bf16) -> fp32 [..., H/factor, W/factor]; factor 2 = [1, 3, 3, 1] / 8 along each
    axis (replicate border) decimated by 2, factor 1 = the conversion to fp32."""
    _dev(x, "x")
    if x.dim() < 2 or factor not in (1, 2):
        raise ValueError(f"flowest_pyr_down: x must be [..., H, W] and factor 1 or 2, got {tuple(x.shape)}, factor {factor!r}")
    H, W = x.shape[-2:]
    if factor == 2 and (H % 2 or W % 2):
        raise ValueError(f"flowest_pyr_down: H = {H} and W = {W} must be even")
    shape = tuple(x.shape[:-2]) + (H // factor, W // factor)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _dev(out, "out")
    assert out.dtype == torch.float32 and tuple(out.shape) == shape
    check(lib.afldm_flowest_pyr_down(ptr(x), ptr(out), x.numel() // (H * W), H, W, factor, _code(x), stream_ptr()), "flowest_pyr_down")
    return out


def flowest_up2(u, out=None):
    """afldm_flowest_up2: fp32 u [..., h, w] -> 2 * bilinear_up2(u) [..., 2h, 2w] (half-pixel centres, clamped)."""
    n, h, w = _flowest_planes(u, "u")
    shape = tuple(u.shape[:-2]) + (2 * h, 2 * w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=u.device)
    assert _flowest_planes(out, "out") == (n, 2 * h, 2 * w)
    check(lib.afldm_flowest_up2(ptr(u), ptr(out), n, h, w, stream_ptr()), "flowest_up2")
    return out


def flowest_smooth(u, out=None):
    """afldm_flowest_smooth: [1, 4, 6, 4, 1] / 16 along each axis of fp32 u [..., H, W], replicate border (not in place)."""
    n, H, W = _flowest_planes(u, "u")
    if out is None:
        out = torch.empty_like(u)
    assert _flowest_planes(out, "out") == (n, H, W)
    check(lib.afldm_flowest_smooth(ptr(u), ptr(out), n, H, W, stream_ptr()), "flowest_smooth")
    return out


def flowest_lk_step(I1, I2, u, radius=3, lam=1e-3, out=None, tile=0):
    """afldm_flowest_lk_step: one damped Lucas-Kanade update of the flow u [B, 2, H, W] (fp32, channel 0 = row displacement)
    for the pair I1, I2 [B, C, H, W] (fp32, C <= 4) in one launch; returns u + du (not in place).  tile: 0 (chosen by the
    call), 16 or 32: the workgroup's output tile; the result does not depend on it."""
    _dev(I1, "I1"); _dev(I2, "I2"); _dev(u, "u")
    if I1.dim() != 4 or I1.shape != I2.shape or I1.dtype != torch.float32 or I2.dtype != torch.float32:
        raise ValueError(f"flowest_lk_step: I1 and I2 must be fp32 [B, C, H, W] of one shape, got {tuple(I1.shape)} and {tuple(I2.shape)}")
    B, C, H, W = I1.shape
    if u.dtype != torch.float32 or tuple(u.shape) != (B, 2, H, W):
        raise ValueError(f"flowest_lk_step: u must be fp32 [{B}, 2, {H}, {W}], got {u.dtype} {tuple(u.shape)}")
    if out is None:
        out = torch.empty_like(u)
    _dev(out, "out")
    assert out.dtype == torch.float32 and out.shape == u.shape
    check(lib.afldm_flowest_lk_step(ptr(I1), ptr(I2), ptr(u), ptr(out), B, C, H, W, int(radius), float(lam), int(tile),
                                    stream_ptr()), "flowest_lk_step")
    return out
