"""ctypes binding of libvamp_post.so (include/vamp_post.h): the posterior summaries.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_post.so")

# name -> (restype, argtypes); mirrors include/vamp_post.h one to one
SIGNATURES = {
    "vamp_post_version": (C.c_int, []),
    "vamp_post_last_error": (C.c_char_p, []),
    "vamp_post_summaries": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int64]
                            + [C.POINTER(C.c_double)] * 9 + [C.POINTER(C.c_int32)] * 2),
}


class PostError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "post", PostError)
