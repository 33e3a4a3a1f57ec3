"""ctypes binding of the lognormal fluor-count fit (C ABI declared in include/fsq_lognormal.h), on the same libfsq_hip.so
handle as _native.  A sibling of _native_chisq."""
import ctypes

from . import _native as N

MAX_FRAMES = 64                 # FSQ_LOGNORMAL_MAX_FRAMES
MAX_POSSIBLE = 15               # FSQ_LOGNORMAL_MAX_POSSIBLE
MAX_BUDGET = 1 << 59            # FSQ_LOGNORMAL_MAX_BUDGET
DEFAULT_BUDGET = 1 << 22        # FSQ_LOGNORMAL_DEFAULT_BUDGET
STATUS_FOUND, STATUS_NONE, STATUS_OVER_BUDGET, STATUS_INVALID = 0, 1, 2, 3


class FsqLognormalParams(ctypes.Structure):
    _fields_ = [("log_fluor_means", ctypes.c_double * (MAX_POSSIBLE + 2)), ("beta_sigma", ctypes.c_double),
                ("max_deviation", ctypes.c_double), ("budget", ctypes.c_int64), ("max_possible", ctypes.c_int32),
                ("allow_multidrop", ctypes.c_int32)]


_P = ctypes.c_void_p
_SIGS = {
    "fsq_lognormal_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "fsq_lognormal_fit": (ctypes.c_int, [_P, _P, _P, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(FsqLognormalParams)] + [_P] * 5 +
                          [_P, ctypes.c_int64, _P]),
    "fsq_lognormal_log": (ctypes.c_int, [_P, _P, ctypes.c_int64, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the lognormal entries bound
