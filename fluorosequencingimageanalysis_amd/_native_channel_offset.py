"""ctypes binding of the estimate of the integer offset between two colour channels (C ABI declared in
include/fsq_channel_offset.h), on the same libfsq_hip.so handle as _native.  A sibling of _native_colocalize."""
import ctypes

from . import _native as N

MAX_W = 64                          # FSQ_CHANNEL_OFFSET_MAX_W: the largest half-width of the histogram of votes
RECORD = 16                         # FSQ_CHANNEL_OFFSET_RECORD: int64 words of the peak's result
MAX_SEGMENT_B = 1 << 24             # a lane whose segment holds this many b's votes nothing: 256 lanes x 2^24 = 2^32

_P, _I64 = ctypes.c_void_p, ctypes.c_int64
_SIGS = {
    "fsq_channel_offset_votes": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P]),
    "fsq_channel_offset_peak": (ctypes.c_int, [_P, _I64, _I64, _I64, _P, _P, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the entries bound
