"""What the ctypes bindings of the side libraries (``_diag_lib``, ``_post_lib``, ``_evid_lib``) and their callers
(``diagnostics``, ``posterior``, ``evidence``) share.

The rules of a binding are those of ``_lib``: no fallback (a missing library raises, every call needs a GPU), and
the library is loaded after torch so that it binds the ROCm runtime torch has mapped -- the one libvamp_hip.so binds
too, so that a device pointer from ``HipContext.run_dev`` means the same thing to every library (INTEGRATION.md,
"Two ROCm runtimes in one process").
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import warnings

import numpy as np

Q_OF_MODE = {0: 3, 1: 4}      # parameters per line: GAUSS3, VOIGT4


def loader(module, stem, error):
    """(bind, load, check) of the binding module named ``module`` for libvamp_<stem>.so.  ``LIB_PATH`` and
    ``SIGNATURES`` are read from the module when the library is loaded (a tool may point ``LIB_PATH`` at another build
    first); ``error`` is what ``check`` raises."""
    name = f"libvamp_{stem}.so"
    loaded = []

    def bind(path):
        lib = C.CDLL(path)
        for fname, (res, args) in sys.modules[module].SIGNATURES.items():
            fn = getattr(lib, fname)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        return lib

    def load():
        if loaded:
            return loaded[0]
        path = sys.modules[module].LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} not found: the HIP extension is not built (run `python -c 'import "
                "__graft_entry__ as g; g.build()'`).  vamp_amd has no CPU fallback.")
        if "torch" not in sys.modules and not os.environ.get("VAMP_NO_IMPORT_ORDER_WARNING"):
            import importlib.util
            try:
                has_torch = importlib.util.find_spec("torch") is not None
            except (ImportError, ValueError):
                has_torch = False
            if has_torch:
                warnings.warn(f"vamp_amd: {name} is being loaded before torch.  If this process imports torch later it "
                              "will hold two ROCm runtimes: `import torch` first (INTEGRATION.md, \"Two ROCm runtimes in one "
                              "process\"); VAMP_NO_IMPORT_ORDER_WARNING=1 silences this.", RuntimeWarning, stacklevel=3)
        loaded.append(bind(path))
        return loaded[0]

    def check(rc, lib=None):
        if rc != 0:
            last_error = getattr(lib or load(), f"vamp_{stem}_last_error")
            raise error(f"libvamp_{stem} error: " + last_error().decode("utf-8", "replace"))

    load.__doc__ = f"Load {name} and attach the prototypes.  Raises if it has not been built."
    return bind, load, check


def region_bases(ctx, chain_ptr):
    """the address of every region's first sample in the device chain ``HipContext.run_dev`` wrote at ``chain_ptr``
    ([n_keep, total_theta] fp64: the regions' [W, D] blocks side by side in a row)"""
    offs = np.concatenate([[0], np.cumsum([int(ctx.W) * d for d in ctx.ndims])]).astype(np.int64)
    return [int(chain_ptr) + 8 * int(o) for o in offs[:-1]]


def fits_with_chain(fits):
    """the ``VPfit`` objects that have been sampled and still hold their device-unit chain"""
    return [f for f in fits if getattr(getattr(f, "mcmc", None), "_fit", None) is not None
            and getattr(f, "_chain_dev", None) is not None]
