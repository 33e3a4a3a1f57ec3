"""ctypes binding of the iterative background correction of signal counts (C ABI declared in include/fsq_background.h and,
for joint signals of several colour channels, include/fsq_background_joint.h), on the
same libfsq_hip.so handle as _native.  A sibling of _native_remainder."""
import ctypes

from . import _native as N

MAX_DROPS = 6                   # FSQ_BACKGROUND_MAX_DROPS
MAX_POSITION = 250              # FSQ_BACKGROUND_MAX_POSITION
MAX_GROUPS = 4096               # FSQ_BACKGROUND_MAX_GROUPS
BATCH_PASSES = 16               # FSQ_BACKGROUND_BATCH_PASSES
TRIAL_THREADS = 64              # FSQ_BACKGROUND_TRIAL_THREADS
TILE = 1024                     # FSQ_BACKGROUND_TILE
RUNNING, NO_DEFINED, THRESHOLD, NO_IMPROVEMENT, CONVERGED, MAX_ITERATIONS, ZERO_TOTAL = range(7)    # FSQ_BACKGROUND_<reason>
OVERFLOW_ACCEPTED, OVERFLOW_UNDEFINED = 1, 2
CAPS = {"FSQ_BACKGROUND_MAX_DROPS": MAX_DROPS, "FSQ_BACKGROUND_MAX_POSITION": MAX_POSITION, "FSQ_BACKGROUND_MAX_GROUPS": MAX_GROUPS,
        "FSQ_BACKGROUND_BATCH_PASSES": BATCH_PASSES, "FSQ_BACKGROUND_TRIAL_THREADS": TRIAL_THREADS, "FSQ_BACKGROUND_TILE": TILE,
        "FSQ_BACKGROUND_RUNNING": RUNNING, "FSQ_BACKGROUND_NO_DEFINED": NO_DEFINED, "FSQ_BACKGROUND_THRESHOLD": THRESHOLD,
        "FSQ_BACKGROUND_NO_IMPROVEMENT": NO_IMPROVEMENT, "FSQ_BACKGROUND_CONVERGED": CONVERGED,
        "FSQ_BACKGROUND_MAX_ITERATIONS": MAX_ITERATIONS, "FSQ_BACKGROUND_ZERO_TOTAL": ZERO_TOTAL,
        "FSQ_BACKGROUND_OVERFLOW_ACCEPTED": OVERFLOW_ACCEPTED, "FSQ_BACKGROUND_OVERFLOW_UNDEFINED": OVERFLOW_UNDEFINED}

JOINT_MAX_DROPS = 8             # FSQ_BACKGROUND_JOINT_MAX_DROPS (include/fsq_background_joint.h)
JOINT_MAX_NEIGHBOURS = 6560     # FSQ_BACKGROUND_JOINT_MAX_NEIGHBOURS
JOINT_MAX_CYCLES = 63           # FSQ_BACKGROUND_JOINT_MAX_CYCLES
JOINT_CAPS = {"FSQ_BACKGROUND_JOINT_MAX_DROPS": JOINT_MAX_DROPS, "FSQ_BACKGROUND_JOINT_MAX_NEIGHBOURS": JOINT_MAX_NEIGHBOURS,
              "FSQ_BACKGROUND_JOINT_MAX_CYCLES": JOINT_MAX_CYCLES}

_P = ctypes.c_void_p
POINTER_FIELDS = ("key_off", "def_off", "first_off", "rest_off", "num_cycles", "include_multidrop", "sigma_threshold", "code",
                  "sorted_code", "sorted_index", "filter", "nb_off", "def_key", "def_avg", "def_std", "und_first", "und_rest",
                  "count", "percent", "rounded", "stop_reason", "n_passes", "n_accepted", "overflow", "accepted_key",
                  "undefined_bp")


class FsqBackgroundArgs(ctypes.Structure):
    _fields_ = ([(k, ctypes.c_int32) for k in ("n_problems", "max_iterations", "max_defined", "accepted_cap", "undefined_cap",
                                               "reserved_")] +
                [(k, ctypes.c_int64) for k in ("n_keys", "n_defined", "n_first", "n_rest", "n_neighbours")] +
                [(k, _P) for k in POINTER_FIELDS])


_SIGS = {
    "fsq_background_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "fsq_background_iterate": (ctypes.c_int, [ctypes.POINTER(FsqBackgroundArgs), _P, ctypes.c_int64, _P]),
}
EXPORTED = tuple(_SIGS)
_JOINT_SIGS = {                     # include/fsq_background_joint.h
    "fsq_background_neighbour_means": (ctypes.c_int, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P]),
}
JOINT_EXPORTED = tuple(_JOINT_SIGS)

lib = N.bind(dict(_SIGS, **_JOINT_SIGS))    # the library handle of _native.lib() with the background entries bound
