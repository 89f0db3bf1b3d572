"""ctypes binding of libvamp_loo.so (include/vamp_loo.h): PSIS-LOO, the leave-one-out predictive density per pixel.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_loo.so")

_OUTPUTS = [C.POINTER(C.c_double)] * 7 + [C.POINTER(C.c_int32)] * 3

# name -> (restype, argtypes); mirrors include/vamp_loo.h one to one
SIGNATURES = {
    "vamp_loo_version": (C.c_int, []),
    "vamp_loo_last_error": (C.c_char_p, []),
    "vamp_loo_pointwise": (C.c_int, [C.c_int, C.c_void_p, C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_int32)] * 4
                           + [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64]
                           + _OUTPUTS + [C.POINTER(C.c_void_p)]),
    "vamp_loo_from_loglik": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.c_int64] + _OUTPUTS),
}


class LooError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "loo", LooError)
