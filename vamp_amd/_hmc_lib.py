"""ctypes binding of libvamp_hmc.so (include/vamp_hmc.h): preconditioned Hamiltonian Monte Carlo chains per region.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_hmc.so")

_PP, _IP, _DP = C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_double)

# name -> (restype, argtypes); mirrors include/vamp_hmc.h one to one
SIGNATURES = {
    "vamp_hmc_version": (C.c_int, []),
    "vamp_hmc_last_error": (C.c_char_p, []),
    "vamp_hmc_chains": (C.c_int, [C.c_int, C.c_void_p, C.c_int] + [_PP] * 3 + [_IP] * 4 + [_PP, _IP, _IP, _IP, _PP, C.c_int, _PP, _DP, _DP]
                        + [C.c_int] * 4 + [C.c_int64, C.c_uint64] + [_PP, _PP, _PP, C.c_int, _PP] + [_IP, _IP, _DP, _DP, _IP, _IP] + [_PP] * 5),
}


class HmcError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "hmc", HmcError)
