"""ctypes binding of the sequence-experiment reduction (C ABI declared in include/fsq_sequence.h), on the same
libfsq_hip.so handle as _native.  Kept apart from _native._SIGS, which mirrors include/fsq.h one to one."""
import ctypes

from . import _native as N

MAX_FRAMES = 64                                 # FSQ_SEQUENCE_MAX_FRAMES
METHOD_MEXICAN_HAT, METHOD_SIMPLE = 0, 1        # FSQ_SEQUENCE_MEXICAN_HAT / _SIMPLE
DETECTED, INTERPOLATED, WINDOW_INSIDE = 1, 2, 4  # bits of the flags output

_PHOTOMETRY = (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                              ctypes.c_void_p] + [ctypes.c_int32] * 5 + [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_void_p])
_SIGS = {
    "fsq_sequence_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]),
    "fsq_sequence_photometry": _PHOTOMETRY,
    "fsq_sequence_photometry_u32": _PHOTOMETRY,
    "fsq_sequence_category_counts_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "fsq_sequence_category_counts": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int64] + [ctypes.c_void_p] * 6 +
                                     [ctypes.c_int64, ctypes.c_void_p]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the sequence entries bound
