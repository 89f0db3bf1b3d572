"""ctypes binding of libvamp_evid.so (include/vamp_evid.h): the log-evidence from tempered ensembles.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_evid.so")

# name -> (restype, argtypes); mirrors include/vamp_evid.h one to one
_DPP = C.POINTER(C.c_void_p)
_DP, _IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
SIGNATURES = {
    "vamp_evid_version": (C.c_int, []),
    "vamp_evid_last_error": (C.c_char_p, []),
    "vamp_evid_default_betas": (C.c_int, [C.c_int, _DP]),
    "vamp_evid_lnlike": (C.c_int, [C.c_int, _DP, _DP, _DP, C.c_int, C.c_int, C.c_int, C.c_int, _DP, C.c_int, _DP, _DP, _DP]),
    "vamp_evid_run": (C.c_int, [C.c_int, C.c_void_p, C.c_int, _DPP, _DPP, _DPP, _IP, _IP, _IP, _IP, _DPP, _IP, C.c_int, _DP, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_uint64, C.c_double, _DPP] + [_DP] * 7 + [_DPP, _DPP, C.c_int, _DP, C.POINTER(C.c_uint8)]),
}


class EvidError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "evid", EvidError)
