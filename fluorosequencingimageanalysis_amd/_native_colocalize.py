"""ctypes binding of the colocalisation of tracks between colour channels (C ABI declared in include/fsq_colocalize.h), on the
same libfsq_hip.so handle as _native.  A sibling of _native_signal_sweep."""
import ctypes

from . import _native as N

MAX_CHANNELS = 4                    # FSQ_PEPTIDE_MAX_CHANNELS: the joint key's letters
MAX_FRAMES = 64                     # FSQ_SIGNAL_MAX_FRAMES
COORD_LIMIT = 1 << 30               # |coordinate| < 2^30: d2 stays below 2^63

_P, _I64 = ctypes.c_void_p, ctypes.c_int64
_SIGS = {
    "fsq_colocalize_match": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the entry bound
