"""ctypes binding of libvamp_relabel.so (include/vamp_relabel.h): the relabelling that undoes label switching.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_relabel.so")

_I32, _F64, _PTRS = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_void_p)

# name -> (restype, argtypes); mirrors include/vamp_relabel.h one to one
SIGNATURES = {
    "vamp_relabel_version": (C.c_int, []),
    "vamp_relabel_last_error": (C.c_char_p, []),
    "vamp_relabel_chains": (C.c_int, [C.c_int, C.c_void_p, C.c_int, _I32, _I32, _I32, _PTRS, C.c_int, C.POINTER(C.c_int64), _I32, _I32,
                                      _PTRS, _PTRS, C.c_int, _PTRS, C.POINTER(C.c_int64), C.c_int, _PTRS, _PTRS, _F64, _F64, _F64]
                            + [_I32] * 5),
    "vamp_relabel_assign": (C.c_int, [C.c_int, C.c_int, C.c_int, _F64, C.POINTER(C.c_uint8), _F64]),
}


class RelabelError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "relabel", RelabelError)
