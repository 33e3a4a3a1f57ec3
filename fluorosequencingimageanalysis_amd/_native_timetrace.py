"""ctypes binding of the timetrace experiment table (C ABI declared in include/fsq_timetrace.h), on the same libfsq_hip.so
handle as _native.  A sibling of _native_stepfit and _native_chisq."""
import ctypes

from . import _native as N

STATUS_ZERO_TSS = 3             # FSQ_TIMETRACE_ZERO_TSS

_P = ctypes.c_void_p
_SIGS = {
    "fsq_timetrace_table": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32] + [_P] * 4 + [_P] * 8 + [_P, _P]),
    "fsq_plateau_values": (ctypes.c_int, [_P] * 4 + [ctypes.c_int64, ctypes.c_int32, _P, _P, _P, _P]),
    "fsq_timetrace_spot_rows": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32, _P, _P]),
    "fsq_timetrace_photometry_rows": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32, _P, _P, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the timetrace entries bound
