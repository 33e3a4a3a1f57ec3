"""ctypes binding of the chi-squared step fitter and the plateau merge filters (C ABI declared in include/fsq_chisq.h), on
the same libfsq_hip.so handle as _native.  A sibling of _native_stepfit, which mirrors include/fsq_stepfit.h one to one."""
import ctypes

from . import _native as N

MAX_FRAMES = 1024               # FSQ_CHISQ_MAX_FRAMES
MERGE_UPSTEPS, MERGE_SMALL_STEPS = 0, 1


class FsqChisqParams(ctypes.Structure):
    _fields_ = [("num_steps", ctypes.c_int32), ("min_step_length", ctypes.c_int32), ("ignore_counterfits", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("num_steps_multiplier", ctypes.c_double), ("min_step_magnitude", ctypes.c_double)]


_P = ctypes.c_void_p
_SIGS = {
    "fsq_chisq_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "fsq_chisq_step_fit": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(FsqChisqParams)] + [_P] * 9 +
                           [ctypes.c_int32, _P, _P, ctypes.c_int64, _P]),
    "fsq_stepfit_merge_filter_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "fsq_stepfit_merge_filter": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32] + [_P] * 4 +
                                 [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, ctypes.c_double] + [_P] * 5 +
                                 [_P, ctypes.c_int64, _P]),
    "fsq_stepfit_r_squared_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "fsq_stepfit_r_squared": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32] + [_P] * 4 + [_P, _P, _P, ctypes.c_int64, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the chi-squared entries bound
