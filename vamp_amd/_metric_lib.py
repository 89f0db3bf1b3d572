"""ctypes binding of libvamp_metric.so (include/vamp_metric.h): a positive-definite metric from any symmetric matrix.

Loading, the torch-order warning and the error check are ``_sidelib``'s, and so are their rules.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvamp_metric.so")

_PP, _IP, _DP, _LP = C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)

# name -> (restype, argtypes); mirrors include/vamp_metric.h one to one.  cov and chol are void*: host or device memory
SIGNATURES = {
    "vamp_metric_version": (C.c_int, []),
    "vamp_metric_last_error": (C.c_char_p, []),
    "vamp_metric_plan": (C.c_int, [C.c_int, _IP, _LP]),
    "vamp_metric_factor": (C.c_int, [C.c_int, C.c_void_p, C.c_int, _PP, C.c_int, _LP, _IP, _IP, _PP, _IP, _DP, _DP, C.c_int, C.c_int,
                                     _DP, _DP, C.c_void_p, _DP, C.c_void_p, _DP, _IP, _IP, _IP, _DP, _IP]),
}


class MetricError(RuntimeError):
    pass


bind, load, check = _sidelib.loader(__name__, "metric", MetricError)
