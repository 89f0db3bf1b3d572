"""ctypes binding of libvamp_laplace.so (include/vamp_laplace.h): importance sampling from a Gaussian proposal, ln Z and
posterior moments with no chain.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_laplace.so")

# name -> (restype, argtypes); mirrors include/vamp_laplace.h one to one
SIGNATURES = {
    "vamp_laplace_version": (C.c_int, []),
    "vamp_laplace_last_error": (C.c_char_p, []),
    "vamp_laplace_points": (C.c_int, [C.c_int, C.c_void_p, C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_int32)] * 4
                            + [C.POINTER(C.c_void_p), C.POINTER(C.c_int32)] + [C.POINTER(C.c_void_p)] * 2 + [C.c_int, C.c_uint64]
                            + [C.POINTER(C.c_double)] * 6 + [C.POINTER(C.c_int32)] * 2 + [C.POINTER(C.c_double)] * 3
                            + [C.POINTER(C.c_void_p)] * 2 + [C.c_int] + [C.POINTER(C.c_void_p)] * 3),
}


class LaplaceError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "laplace", LaplaceError)
