"""ctypes binding of the sequence-experiment glue (C ABI declared in include/fsq_experiment.h), on the same libfsq_hip.so
handle as _native.  Kept apart from _native._SIGS, which mirrors include/fsq.h one to one."""
import ctypes

from . import _native as N

STATUS_OK, STATUS_REKEY_ASSERT, STATUS_INVALID = 0, 1, 2        # FSQ_EXPERIMENT_* of the spot table's per-frame status
SPOT_SIZE = 5                                                   # the size of every Spot made from a fit (fit_img is 5 x 5)

_SIGS = {
    "fsq_experiment_spot_table_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "fsq_experiment_spot_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p] +
                                  [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 7 + [ctypes.c_int64, ctypes.c_void_p]),
    "fsq_experiment_trace_starts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    "fsq_experiment_trace_rows": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64] +
                                  [ctypes.c_void_p] * 4),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the experiment entries bound
