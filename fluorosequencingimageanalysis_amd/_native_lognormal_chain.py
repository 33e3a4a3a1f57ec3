"""ctypes binding of the per-track steps between the two fits of the lognormal chain (C ABI declared in
include/fsq_lognormal_chain.h), on the same libfsq_hip.so handle as _native.  A sibling of _native_remainder."""
import ctypes

from . import _native as N

MAX_FRAMES = 64                 # FSQ_CHAIN_MAX_FRAMES

_P = ctypes.c_void_p
_WS = (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64])
_SIGS = {
    "fsq_chain_last_drops_workspace_bytes": _WS,
    "fsq_chain_on_off_medians_workspace_bytes": _WS,
    "fsq_chain_on_off_adjust_workspace_bytes": _WS,
    "fsq_chain_last_drops": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _P, _P, _P, ctypes.c_int64, _P,
                                            ctypes.c_int64, _P]),
    "fsq_chain_on_off_medians": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_double, _P, _P,
                                                _P, _P, ctypes.c_int64, _P]),
    "fsq_chain_on_off_adjust": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_double, _P, _P, _P, _P,
                                               _P, ctypes.c_int64, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the chain entries bound
