"""ctypes binding of libvamp_fisher.so (include/vamp_fisher.h): gradient, information matrix and covariance at given
points from the analytic Jacobian.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_fisher.so")

# name -> (restype, argtypes); mirrors include/vamp_fisher.h one to one
SIGNATURES = {
    "vamp_fisher_version": (C.c_int, []),
    "vamp_fisher_last_error": (C.c_char_p, []),
    "vamp_fisher_points": (C.c_int, [C.c_int, C.c_void_p, C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_int32)] * 4
                           + [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int]
                           + [C.POINTER(C.c_double)] * 6 + [C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
}


class FisherError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "fisher", FisherError)
