"""ctypes binding of libafldm_edit.so - the slot sampler's update for image-conditioned requests (include/afldm_hip_edit.h:
afldm_slot_step_edit), bound from that header (_lib.EDIT_ABI) like the product library's.

The library is built with the product library and links against it.  It is loaded on first use - by ops.slot_step_edit, that is
by an EditSlotEngine - and there is nothing behind it: a missing library is an error."""
import ctypes
import os

from ._lib import EDIT_ABI, LIB_PATH

EDIT_PATH = os.environ.get("AFLDM_EDIT_LIB") or os.path.join(os.path.dirname(LIB_PATH), "libafldm_edit.so")
_state = {}


def lib():
    """The loaded library (raises ImportError when it was not built)."""
    if "lib" not in _state:
        if not os.path.exists(EDIT_PATH):
            raise ImportError(f"{EDIT_PATH} is missing: run `python -m afldm_amd.build` (hipcc, gfx950). afldm_amd has no fallback "
                              "for the edit slots' update kernel.")
        h = ctypes.CDLL(EDIT_PATH, mode=ctypes.RTLD_GLOBAL)
        _state["exports"] = EDIT_ABI.bind(h)
        _state["lib"] = h
    return _state["lib"]


def exports():
    lib()
    return _state["exports"]
