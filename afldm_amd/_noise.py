"""ctypes binding of libafldm_noise.so - counter-based device noise and the seeded samplers' updates (include/afldm_hip_noise.h:
afldm_philox_bits, afldm_counter_noise, afldm_seeded_step, afldm_slot_step_seeded), bound from that header (_lib.NOISE_ABI) like
the product library's.

The library is built with the product library and links against it.  It is loaded on first use - by ops.philox_bits,
ops.counter_noise, ops.seeded_step and ops.slot_step_seeded, that is by a SeededEngine or a SeededSlotEngine - and there is
nothing behind it: a missing library is an error."""
import ctypes
import os

from ._lib import LIB_PATH, NOISE_ABI

NOISE_PATH = os.environ.get("AFLDM_NOISE_LIB") or os.path.join(os.path.dirname(LIB_PATH), "libafldm_noise.so")
_state = {}


def lib():
    """The loaded library (raises ImportError when it was not built)."""
    if "lib" not in _state:
        if not os.path.exists(NOISE_PATH):
            raise ImportError(f"{NOISE_PATH} is missing: run `python -m afldm_amd.build` (hipcc, gfx950). afldm_amd has no fallback "
                              "for the counter-based noise kernels.")
        h = ctypes.CDLL(NOISE_PATH, mode=ctypes.RTLD_GLOBAL)
        _state["exports"] = NOISE_ABI.bind(h)
        _state["lib"] = h
    return _state["lib"]


def exports():
    lib()
    return _state["exports"]
