"""ctypes binding of libafldm_hip.so, derived at import from include/afldm_hip.h.

The header is the one description of the C ABI: _abi.py reads its prototypes, argument structs, enums and #defines, and
every argtypes / restype, ConvArgs / SepArgs / AfActArgs and F32 / BF16 below come from there.  A new entry point needs its
prototype in the header and nothing here; a declaration the reader does not understand fails the import, naming the type.
Every pointer that is not `char*` or an argument struct is a c_void_p: a device address (tensor.data_ptr(), None = NULL), or
for the few host arrays (filter_matrix's output, the route queries, origin lists, blur taps) a ctypes array.

The library is the ONLY compute path of afldm_amd: if it cannot be loaded, importing this
module raises — there is no CPU fallback."""
import ctypes
import os
from ctypes import c_float

import torch  # noqa: F401  (imported first so torch's libamdhip64.so.7 is the one HIP runtime in-process)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# AFLDM_LIB: alternative build of the same library (A/B timing of kernel changes on one GPU box)
LIB_PATH = os.environ.get("AFLDM_LIB") or os.path.join(_HERE, "lib", "libafldm_hip.so")

ABI = _abi.read("afldm_hip.h")
# the experiments' declarations (and their afldm_af_act_args) are read here too, so that they need no library: _exp.py binds
# libafldm_exp.so from EXP_ABI on first use
EXP_ABI = _abi.read("afldm_hip_experimental.h", ABI)
# the slot sampler's extension (libafldm_slots.so): bound by _slots.py on first use
SLOTS_ABI = _abi.read("afldm_hip_slots.h", ABI)
# counter-based device noise and the seeded samplers' updates (libafldm_noise.so): bound by _noise.py on first use
NOISE_ABI = _abi.read("afldm_hip_noise.h", ABI)
# the slot sampler's update for image-conditioned requests (libafldm_edit.so): bound by _edit.py on first use
EDIT_ABI = _abi.read("afldm_hip_edit.h", ABI)
ConvArgs, SepArgs, AfActArgs = ABI.structs["afldm_conv_args"], ABI.structs["afldm_sep_args"], EXP_ABI.structs["afldm_af_act_args"]
F32, BF16 = ABI.constants["AFLDM_F32"], ABI.constants["AFLDM_BF16"]
DTYPE_CODE = {torch.float32: F32, torch.bfloat16: BF16}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: run `python -m afldm_amd.build` (hipcc, gfx950). "
            "afldm_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    return lib, ABI.bind(lib)      # AttributeError here = header/library mismatch


lib, EXPORTS = _load()


class AfldmError(RuntimeError):
    pass


_HASH = []


def library_hash():
    """sha256 of the loaded library file, read once: what identifies the build (a ReversibleCode records it, because another
    build's kernels may round differently)."""
    if not _HASH:
        import hashlib
        with open(LIB_PATH, "rb") as f:
            _HASH.append(hashlib.sha256(f.read()).hexdigest())
    return _HASH[0]


def check(rc, what=""):
    if rc != 0:
        msg = lib.afldm_last_error()
        raise AfldmError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def filter_matrix(kind: int, N: int, up: int = 2) -> torch.Tensor:
    """Host fp32 matrix: kind 0 -> U [up*N, N]; kind 1 -> D [N/2, N]; kind 2 -> L [N, N]."""
    rows, cols = {0: (up * N, N), 1: (N // 2, N), 2: (N, N)}[kind]
    buf = (c_float * (rows * cols))()
    check(lib.afldm_filter_matrix(kind, N, up, buf), "afldm_filter_matrix")
    return torch.frombuffer(buf, dtype=torch.float32).clone().reshape(rows, cols)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream
