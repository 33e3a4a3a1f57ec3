"""ctypes binding of the histogram bin search of the lognormal chain (C ABI declared in include/fsq_binsearch.h), on the same
libfsq_hip.so handle as _native.  A sibling of _native_lognormal."""
import ctypes

from . import _native as N

MAX_BINS = 10000                # FSQ_BINSEARCH_MAX_BINS

_P = ctypes.c_void_p
_SIGS = {
    "fsq_histogram_costs": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P, ctypes.c_int, _P, _P]),
    "fsq_histogram_costs_sorted": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, _P, _P]),
    "fsq_histogram_counts": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_int, _P, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the bin-search entries bound
