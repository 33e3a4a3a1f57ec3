"""ctypes binding of the proteome Monte-Carlo (C ABI declared in include/fsq_proteome_mc.h), on the same libfsq_hip.so handle as
_native.  A sibling of _native_signal_sweep."""
import ctypes

from . import _native as N

STREAM = 3                          # FSQ_PMC_STREAM
MAX_ACIDS = 8                       # FSQ_PMC_MAX_ACIDS
MAX_LABELS = 64                     # FSQ_PMC_MAX_LABELS
MAX_HEAD = 255                      # FSQ_PMC_MAX_HEAD
MAX_ROW = 4096                      # FSQ_PMC_MAX_ROW
MAX_EXPOSURES = 64                  # FSQ_PMC_MAX_EXPOSURES
MAX_SIGNAL_SLOTS = 1 << 27          # FSQ_PMC_MAX_SIGNAL_SLOTS
MAX_PAIR_SLOTS = 1 << 28            # FSQ_PMC_MAX_PAIR_SLOTS
BLOCK, MAX_BLOCKS = 256, 2048       # kpm_signals' and kpm_tally's grid: one pass covers BLOCK * MAX_BLOCKS rows
RATIO_NONE, RATIO_NUMBER, RATIO_ABSENT = 0, 1, 2        # FSQ_PMC_RATIO_*
PROJECT, WITHIN, MASK_MAJOR = 0, 1, 0x100               # FSQ_PMC_PROJECT, FSQ_PMC_WITHIN, FSQ_PMC_MASK_MAJOR
MAX_MASKS = 4096                    # FSQ_PMC_MAX_MASKS
MAX_POINTS = 4096                   # FSQ_PMC_MAX_POINTS


class FsqProteomeParams(ctypes.Structure):
    _fields_ = [("E", ctypes.c_uint64 * MAX_ACIDS), ("O", ctypes.c_uint64 * MAX_ACIDS), ("base", ctypes.c_int32 * MAX_ACIDS),
                ("n_acids", ctypes.c_int32), ("max_d", ctypes.c_int32), ("u", ctypes.c_double), ("seed", ctypes.c_uint64),
                ("first_sample", ctypes.c_uint64), ("sample_size", ctypes.c_int64)]


class FsqUniquesParams(ctypes.Structure):
    _fields_ = [("worst_ratio", ctypes.c_double), ("absolute_min", ctypes.c_double), ("maximum_secondary", ctypes.c_double),
                ("ratio_mode", ctypes.c_int32), ("has_maximum_secondary", ctypes.c_int32), ("demote", ctypes.c_int32),
                ("reserved_", ctypes.c_int32)]


class FsqProteomePoint(ctypes.Structure):
    _fields_ = [("u", ctypes.c_double), ("edman_table", ctypes.c_int32), ("bleach_table", ctypes.c_int32)]


assert ctypes.sizeof(FsqProteomeParams) == 200 and ctypes.sizeof(FsqUniquesParams) == 40 and ctypes.sizeof(FsqProteomePoint) == 16

_P, _I64 = ctypes.c_void_p, ctypes.c_int64
_SIGS = {
    "fsq_proteome_signals": (ctypes.c_int, [ctypes.POINTER(FsqProteomeParams), _P, _P, _P, _P, _I64, _P, _P, _P, _I64, _I64, _P, _P, _P,
                                            _P]),
    "fsq_proteome_tally": (ctypes.c_int, [_P, _P, _I64, _P, _I64, _P, _P, _I64, _P, _P]),
    "fsq_proteome_project": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, ctypes.c_int32, _P, _I64, _P, _P, _I64, _P, _P]),
    "fsq_proteome_signals_points": (ctypes.c_int, [ctypes.POINTER(FsqProteomeParams), _P, _I64, _I64, _P, _P, _P, _P, _I64, _P, _P,
                                                   ctypes.c_int32, _P, ctypes.c_int32, _I64, _I64, _P, _P, _P, _P]),
    "fsq_proteome_tally_points": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _I64, _P, _P, _I64, _P, _P]),
    "fsq_proteome_uniques": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(FsqUniquesParams), _P, _P, _P, _P, _P, _P, _P, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the proteome entries bound
