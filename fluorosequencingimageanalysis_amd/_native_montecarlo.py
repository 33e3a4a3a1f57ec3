"""ctypes binding of the seeded Monte-Carlo PSF fit (C ABI declared in include/fsq_montecarlo.h), on the same libfsq_hip.so
handle as _native.  A sibling of _native_peptide_sim."""
import ctypes

from . import _native as N

MC_OK, MC_NEVER_IMPROVED, MC_NO_MAXIMUM = 0, 1, 2       # FSQ_MC_*
MAX_N_ITER = 2 ** 31 - 1

_P = ctypes.c_void_p
_SIGS = {
    "fsq_mc_fit_rois": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, _P, _P, _P, _P, _P]),
    "fsq_mc_fit_candidates": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_uint64, ctypes.c_int64, _P, _P, _P, _P, _P]),
    "fsq_find_peptides_mc_workspace_bytes": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64]),
    "fsq_find_peptides_mc": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(N.FsqDetectParams),
                                            ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64,
                                            ctypes.c_int64, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P,
                                            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), _P, ctypes.c_int64, _P]),
}
EXPORTED = tuple(_SIGS)

lib = N.bind(_SIGS)                 # the library handle of _native.lib() with the Monte-Carlo entries bound
