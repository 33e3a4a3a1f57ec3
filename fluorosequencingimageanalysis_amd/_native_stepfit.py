"""ctypes binding of the trace step fit (C ABI declared in include/fsq_stepfit.h), on the same libfsq_hip.so handle as
_native.  Kept apart from _native._SIGS, which mirrors include/fsq.h one to one."""
import ctypes

from . import _native as N

MAX_WINDOWS = 16                # FSQ_STEPFIT_MAX_WINDOWS
MAX_MIRRORED = 8192             # FSQ_STEPFIT_MAX_MIRRORED
STATUS_OK, STATUS_UNSUPPORTED, STATUS_INVALID = 0, 1, 2


class FsqStepfitParams(ctypes.Structure):
    _fields_ = [("mirror_start", ctypes.c_int32), ("chung_kennedy", ctypes.c_int32), ("n_windows", ctypes.c_int32),
                ("window_lengths", ctypes.c_int32 * MAX_WINDOWS), ("M", ctypes.c_int32), ("p", ctypes.c_int32),
                ("window_radius", ctypes.c_int32), ("drop_sort", ctypes.c_int32), ("p_threshold", ctypes.c_double),
                ("has_photometry_min", ctypes.c_int32), ("photometry_min", ctypes.c_double)]


_SIGS = {
    "fsq_stepfit_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(FsqStepfitParams)]),
    "fsq_stepfit_traces": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                          ctypes.POINTER(FsqStepfitParams)] + [ctypes.c_void_p] * 13 +
                           [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "fsq_stepfit_ttest_filter_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "fsq_stepfit_ttest_filter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32] +
                                 [ctypes.c_void_p] * 4 + [ctypes.c_double, ctypes.c_int32, ctypes.c_int32] +
                                 [ctypes.c_void_p] * 7 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the step-fit entries bound
