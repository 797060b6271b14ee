"""ctypes binding of libafldm_exp.so - the EXPERIMENTAL entry points of include/afldm_hip_experimental.h, bound from that
header (_lib.EXP_ABI) like the product library's.

Not part of the product: merged activation / convolution launches, the cooperative 2x2-level trunk and the fused small-plane
attention were built, validated and measured slower (profiles/r05/); nothing on the default path imports this module's
library - it is loaded on first use by the opt-in switches (AFLDM_TRUNK, AFLDM_ATTN_SMALL_T), the A/B tools
and the tests that keep the experiments correct."""
import ctypes
import os

from ._lib import EXP_ABI, LIB_PATH

EXP_PATH = os.environ.get("AFLDM_EXP_LIB") or os.path.join(os.path.dirname(LIB_PATH), "libafldm_exp.so")
_state = {}


def available():
    return os.path.exists(EXP_PATH)


def lib():
    """The loaded experimental library (raises ImportError when it was not built)."""
    if "lib" not in _state:
        if not available():
            raise ImportError(f"{EXP_PATH} is missing: run `python -m afldm_amd.build` (the experiments are optional; the product "
                              "library does not need them)")
        h = ctypes.CDLL(EXP_PATH, mode=ctypes.RTLD_GLOBAL)
        _state["exports"] = EXP_ABI.bind(h)
        _state["lib"] = h
    return _state["lib"]


def exports():
    lib()
    return _state["exports"]
