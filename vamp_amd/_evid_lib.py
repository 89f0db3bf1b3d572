"""ctypes binding of libvamp_evid.so (include/vamp_evid.h): the log-evidence from tempered ensembles.

The same rules as ``_lib``, ``_diag_lib`` and ``_post_lib``: no fallback (a missing library raises, every call needs a GPU),
and the library is loaded after torch so that it binds the ROCm runtime torch has mapped -- the one
libvamp_hip.so binds too, so that a device pointer from ``HipContext.run_dev`` means the same thing to
every library ("Two ROCm runtimes in one process").
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import warnings

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvamp_evid.so")

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

_lib = None


def bind(path):
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load libvamp_evid.so and attach the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built (run `python -c 'import "
            "__graft_entry__ as g; g.build()'`).  vamp_amd has no CPU fallback.")
    if "torch" not in sys.modules and not os.environ.get("VAMP_NO_IMPORT_ORDER_WARNING"):
        import importlib.util
        try:
            has_torch = importlib.util.find_spec("torch") is not None
        except (ImportError, ValueError):
            has_torch = False
        if has_torch:
            warnings.warn("vamp_amd: libvamp_evid.so is being loaded before torch.  If this process imports torch later it "
                          "will hold two ROCm runtimes: `import torch` first (INTEGRATION.md, \"Two ROCm runtimes in one "
                          "process\"); VAMP_NO_IMPORT_ORDER_WARNING=1 silences this.", RuntimeWarning, stacklevel=3)
    _lib = bind(LIB_PATH)
    return _lib


class EvidError(RuntimeError):
    pass


def check(rc, lib=None):
    if rc != 0:
        raise EvidError("libvamp_evid error: " + (lib or load()).vamp_evid_last_error().decode("utf-8", "replace"))
