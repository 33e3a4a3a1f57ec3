"""ctypes binding of the remainder correction of track photometries (C ABI declared in include/fsq_remainder.h), on the same
libfsq_hip.so handle as _native.  A sibling of _native_binsearch."""
import ctypes

from . import _native as N

MAX_FRAMES = 64                 # FSQ_REMAINDER_MAX_FRAMES
LDS_MAX = 512                   # FSQ_REMAINDER_LDS_MAX
MODE_RATIO, MODE_ADDITIVE = 0, 1


class FsqRemainderParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("minimum_r_per_field", ctypes.c_int32)]


_P = ctypes.c_void_p
_SIGS = {
    "fsq_remainder_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64]),
    "fsq_remainder_adjust": (ctypes.c_int, [_P, _P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                            ctypes.POINTER(FsqRemainderParams), _P, _P, _P, _P, _P, ctypes.c_int64, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the remainder entries bound
