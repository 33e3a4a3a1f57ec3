"""ctypes binding of the peptide Monte-Carlo simulation (C ABI declared in include/fsq_peptide_sim.h), on the same
libfsq_hip.so handle as _native.  A sibling of _native_lognormal."""
import ctypes

from . import _native as N

MAX_LENGTH = 64                 # FSQ_PEPTIDE_MAX_LENGTH
MAX_LABELLED = 15               # FSQ_PEPTIDE_MAX_LABELLED
MAX_FRAMES = 64                 # FSQ_PEPTIDE_MAX_FRAMES
CAUSE_NONE, CAUSE_DUD, CAUSE_DESTRUCTION, CAUSE_EDMAN, CAUSE_STRIP = 0, 1, 2, 3, 4
OFF_LOG = -10000.0              # FSQ_PEPTIDE_OFF_LOG


class FsqPeptideSimParams(ctypes.Structure):
    _fields_ = [("label_mask", ctypes.c_uint64), ("seed", ctypes.c_uint64), ("first_molecule", ctypes.c_int64),
                ("p", ctypes.c_double), ("per_cycle_b", ctypes.c_double), ("u", ctypes.c_double), ("s", ctypes.c_double),
                ("s2", ctypes.c_double), ("log_beta", ctypes.c_double), ("beta_sigma", ctypes.c_double),
                ("superdye_rate", ctypes.c_double), ("superdye_factor", ctypes.c_double),
                ("ddif", ctypes.c_double * MAX_LABELLED), ("n_ddif", ctypes.c_int32), ("length", ctypes.c_int32),
                ("num_mocks", ctypes.c_int32), ("num_edmans", ctypes.c_int32), ("sc", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


assert ctypes.sizeof(FsqPeptideSimParams) == 240

_P = ctypes.c_void_p
_SIGS = {
    "fsq_peptide_simulate": (ctypes.c_int, [ctypes.POINTER(FsqPeptideSimParams), ctypes.c_int64] + [_P] * 8 + [_P]),
    "fsq_philox_words": (ctypes.c_int, [_P, _P, ctypes.c_int64, _P, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the simulation entries bound
