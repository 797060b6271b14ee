"""ctypes binding of libafldm_slots.so - the slot sampler's update for mixed solvers (include/afldm_hip_slots.h:
afldm_slot_step_kinds), bound from that header (_lib.SLOTS_ABI) like the product library's.

The library is built with the product library and links against it.  It is loaded on first use - by ops.slot_step_kinds, that
is by a SlotEngine built with kinds other than ("ddim",) - and there is nothing behind it: a missing library is an error."""
import ctypes
import os

from ._lib import LIB_PATH, SLOTS_ABI

SLOTS_PATH = os.environ.get("AFLDM_SLOTS_LIB") or os.path.join(os.path.dirname(LIB_PATH), "libafldm_slots.so")
_state = {}


def lib():
    """The loaded library (raises ImportError when it was not built)."""
    if "lib" not in _state:
        if not os.path.exists(SLOTS_PATH):
            raise ImportError(f"{SLOTS_PATH} is missing: run `python -m afldm_amd.build` (hipcc, gfx950). afldm_amd has no fallback "
                              "for afldm_slot_step_kinds.")
        h = ctypes.CDLL(SLOTS_PATH, mode=ctypes.RTLD_GLOBAL)
        _state["exports"] = SLOTS_ABI.bind(h)
        _state["lib"] = h
    return _state["lib"]


def exports():
    lib()
    return _state["exports"]
