"""ctypes binding of the simulation parameter sweep (C ABI declared in include/fsq_signal_sweep.h), on the same
libfsq_hip.so handle as _native.  A sibling of _native_peptide_sim."""
import ctypes

from . import _native as N
from ._native_peptide_labels import FsqPeptideLabelsParams
from ._native_peptide_sim import FsqPeptideSimParams

MAX_DROPS = 10                      # FSQ_SIGNAL_MAX_DROPS
MAX_FRAMES = 64                     # FSQ_SIGNAL_MAX_FRAMES
JOINT_DROP_BITS = {1: 6, 2: 7, 3: 8, 4: 8}      # FSQ_SIGNAL_JOINT_DROP_BITS(K)
JOINT_MAX_DROPS = {1: 10, 2: 8, 3: 6, 4: 6}     # FSQ_SIGNAL_JOINT_MAX_DROPS(K)
EMPTY = 0x400                       # FSQ_SIGNAL_EMPTY
NEVER = 0x800                       # FSQ_SIGNAL_NEVER
MAX_SLOTS = 1 << 24                 # FSQ_SIGNAL_MAX_SLOTS
MAX_COUNT = (1 << 31) - 1           # what fsq_signal_scores takes as a count
MAX_SEL = 2048                      # FSQ_SIGNAL_PAIR_MAX_SEL

METRICS = ('naive', 'my_euclidean', 'normalized_euclidean', 'my_std_normalized_euclidean', 'my_sim_std_normalized_euclidean',
           'log_rmsd', 'my_canberra', 'my_chebyshev', 'my_normalized_chebyshev', 'my_std_normalized_chebyshev')   # FSQ_SCORE_*
NORMALIZE_COUNTS, HEATMAP_NORMALIZE_COUNTS = 1, 2
SCORE_OK, SCORE_EMPTY, SCORE_DIVZERO, SCORE_DOMAIN = 0, 1, 2, 3


class FsqSweepPoint(ctypes.Structure):
    _fields_ = [("p", ctypes.c_double), ("per_cycle_b", ctypes.c_double), ("u", ctypes.c_double), ("s", ctypes.c_double),
                ("s2", ctypes.c_double)]


class FsqScoreParams(ctypes.Structure):
    _fields_ = [("n_observed", ctypes.c_int64), ("small_count_cutoff", ctypes.c_double), ("has_cutoff", ctypes.c_int32),
                ("normalization", ctypes.c_int32), ("metric", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


assert ctypes.sizeof(FsqSweepPoint) == 40 and ctypes.sizeof(FsqScoreParams) == 32

_P, _I64, _I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
_SIGS = {
    "fsq_peptide_simulate_points": (ctypes.c_int, [ctypes.POINTER(FsqPeptideSimParams), _P, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _P]),
    "fsq_signal_tally": (ctypes.c_int, [_P, _I32, _P, _P, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    # (declared in fsq_signal_sweep.h beside fsq_peptide_simulate_points, defined in fsq_peptide_labels.hip)
    "fsq_peptide_simulate_labels_points": (ctypes.c_int, [ctypes.POINTER(FsqPeptideLabelsParams), _P, _I64, _I64, _I64, _I64, _I64, _P, _P,
                                                          _P, _P]),
    "fsq_signal_tally_joint": (ctypes.c_int, [_P, _I32, _I32, _P, _P, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "fsq_signal_lookup": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32, _P, _P]),
    "fsq_signal_scores": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _I32, _I32, ctypes.POINTER(FsqScoreParams), _P, _P, _P, _P, _P]),
    "fsq_signal_pair_best": (ctypes.c_int, [_P, _P, _P, _P, _P, _I32, _I32, ctypes.POINTER(FsqScoreParams), _P, _I32, _I32, _P, _P,
                                            _P, _P, _P, _P, _P, _P, _P]),
    "fsq_signal_pair_extremes": (ctypes.c_int, [_P, _I32, _I32, _P, _P, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the sweep's entries bound
