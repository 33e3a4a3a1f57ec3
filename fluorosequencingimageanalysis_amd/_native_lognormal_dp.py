"""ctypes binding of the lognormal fit by exact dynamic programme (C ABI declared in include/fsq_lognormal_dp.h), on the same
libfsq_hip.so handle as _native.  A sibling of _native_lognormal, whose FsqLognormalParams and status codes it reuses."""
import ctypes

from . import _native as N
from ._native_lognormal import FsqLognormalParams

_P = ctypes.c_void_p
_SIGS = {
    "fsq_lognormal_dp_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "fsq_lognormal_fit_dp": (ctypes.c_int, [_P, _P, _P, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(FsqLognormalParams)] + [_P] * 5 +
                             [ctypes.c_int32, _P, ctypes.c_int64, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the entries bound
