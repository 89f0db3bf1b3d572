"""ctypes binding of libvamp_diag.so (include/vamp_diag.h): the chain diagnostics.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_diag.so")

# name -> (restype, argtypes); mirrors include/vamp_diag.h one to one
SIGNATURES = {
    "vamp_diag_version": (C.c_int, []),
    "vamp_diag_last_error": (C.c_char_p, []),
    "vamp_diag_chains": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_double,
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]),
}


class DiagError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "diag", DiagError)
