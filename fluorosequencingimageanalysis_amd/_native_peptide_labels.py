"""ctypes binding of the peptide Monte-Carlo simulation for several label letters (C ABI declared in
include/fsq_peptide_labels.h), on the same libfsq_hip.so handle as _native.  A sibling of _native_peptide_sim."""
import ctypes

from . import _native as N
from ._native_peptide_sim import MAX_FRAMES, MAX_LABELLED, MAX_LENGTH       # noqa: F401  (the limits of fsq_peptide_sim.h hold)

MAX_CHANNELS = 4                # FSQ_PEPTIDE_MAX_CHANNELS

_D4 = ctypes.c_double * MAX_CHANNELS


class FsqPeptideLabelsParams(ctypes.Structure):
    _fields_ = [("channel_mask", ctypes.c_uint64 * MAX_CHANNELS), ("seed", ctypes.c_uint64), ("first_molecule", ctypes.c_int64),
                ("p", ctypes.c_double), ("per_cycle_b", ctypes.c_double), ("u", ctypes.c_double), ("s", ctypes.c_double),
                ("s2", ctypes.c_double), ("log_beta", _D4), ("beta_sigma", _D4), ("superdye_rate", _D4), ("superdye_factor", _D4),
                ("ddif", (ctypes.c_double * MAX_LABELLED) * MAX_CHANNELS), ("n_ddif", ctypes.c_int32 * MAX_CHANNELS),
                ("n_channels", ctypes.c_int32), ("length", ctypes.c_int32), ("num_mocks", ctypes.c_int32),
                ("num_edmans", ctypes.c_int32), ("sc", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


assert ctypes.sizeof(FsqPeptideLabelsParams) == 736


_P = ctypes.c_void_p
_SIGS = {
    "fsq_peptide_simulate_labels": (ctypes.c_int, [ctypes.POINTER(FsqPeptideLabelsParams), ctypes.c_int64] + [_P] * 8 + [_P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the entry bound
