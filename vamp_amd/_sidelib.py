"""What the ctypes bindings of the side libraries (``_diag_lib``, ``_post_lib``, ``_evid_lib``, ``_pred_lib``,
``_loo_lib``, ``_relabel_lib``, ``_fisher_lib``, ``_laplace_lib``) and their callers (``diagnostics``, ``posterior``,
``evidence``, ``predictive``, ``loo``, ``relabel``, ``fisher``, ``laplace``) share; the second part is what the callers that walk every sample of a
chain (``posterior``, ``predictive``, ``loo``, ``relabel``) hand their libraries alike; the third is what the two that
evaluate the pointwise log-likelihood (``predictive``, ``loo``) do alike around their library call.

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
MAX_CHAIN_SAMPLES = 16384     # VAMP_POST_MAX_SAMPLES of include/vamp_post.h, VAMP_PRED_MAX_SAMPLES of include/vamp_pred.h


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


# ---- the chain arguments of vamp_post_summaries and vamp_pred_pointwise ------------------------------------------
def per_group(v, G, cast):
    """one value for all ``G`` groups, or one per group"""
    return [cast(v)] * G if np.isscalar(v) else [cast(e) for e in v]


def time_step(n_keep, walkers):
    """the smallest step s for which every s-th of ``n_keep`` kept samples of ``walkers`` walkers fits the libraries:
    ceil(n_keep / s) * walkers <= MAX_CHAIN_SAMPLES"""
    if walkers > MAX_CHAIN_SAMPLES:
        raise ValueError(f"an ensemble of {walkers} walkers exceeds the {MAX_CHAIN_SAMPLES} samples the library takes")
    rows = MAX_CHAIN_SAMPLES // walkers
    step = max(1, -(-n_keep // rows))
    while -(-n_keep // step) > rows:
        step += 1
    return step


def check_chain_shapes(arrays, n_comp, modes, sds, notes):
    """every chain is [N, W, D] with the D of its lines and mode; ``notes[g]`` closes the message"""
    for a, k, m, sd, note in zip(arrays, n_comp, modes, sds, notes):
        if a.ndim != 3:
            raise ValueError("every chain must be an [N, W, D] array")
        if m in Q_OF_MODE and a.shape[2] != Q_OF_MODE[m] * k + sd:
            raise ValueError(f"a chain of {a.shape[2]} parameters does not hold {k} lines of mode {m} ({note})")


def host_layout(arrays, steps):
    """(bases, ld, n_keep, walkers) of contiguous fp64 [N, W, D] host arrays, every ``steps[g]``-th time read in place"""
    return ([a.ctypes.data for a in arrays], [a.shape[1] * a.shape[2] * s for a, s in zip(arrays, steps)],
            [-(-a.shape[0] // s) for a, s in zip(arrays, steps)], [a.shape[1] for a in arrays])


def context_layout(ctx, chain_ptr, n_keep):
    """(n_comp, modes, sample_sd, bases, ld, n_keep, walkers) of the regions of the device chain ``HipContext.run_dev``
    wrote at ``chain_ptr``"""
    R, mode = len(ctx.ndims), int(ctx.mode)
    ks = [int(k) for k in ctx.n_comp]
    sds = [d - Q_OF_MODE.get(mode, 3) * k for d, k in zip(ctx.ndims, ks)]
    return ks, [mode] * R, sds, region_bases(ctx, chain_ptr), [ctx.total_theta] * R, [int(n_keep)] * R, [int(ctx.W)] * R


def chain_args(n_pix, n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers):
    """the arguments n_pix .. walkers of both entry points, in the headers' order, as ctypes takes them (a pointer keeps
    its array alive)"""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return [i32(n_pix), i32(n_comp), i32(modes), i32(sample_sd), (C.c_void_p * len(bases))(*[int(b) for b in bases]),
            int(bool(is_device)), np.ascontiguousarray(ld, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64)), i32(n_keep), i32(walkers)]


# ---- around vamp_pred_pointwise and vamp_loo_pointwise: the data, the outputs, the records ----------------------------
def data_args(xs, fluxes, noises):
    """(xs, fluxes, noises) as contiguous fp64 arrays (a noise of None stays None); a group's have one shape"""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    xs, fluxes = [f64(x) for x in xs], [f64(f) for f in fluxes]
    noises = [None if n is None else f64(n) for n in noises]
    for x, f, n in zip(xs, fluxes, noises):
        if f.shape != x.shape or (n is not None and n.shape != x.shape):
            raise ValueError("flux and noise must have the abscissa's shape")
    return xs, fluxes, noises


def pointer_array(arrays):
    """a ``const double* const*`` of host arrays (None: NULL)"""
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def outputs(G, tot_pix, want, pix, grp, cnt):
    """(the output arrays by name, the output arguments in the header's order) of a call over ``G`` groups of ``tot_pix``
    pixels: of the per-pixel (``pix``), per-group (``grp``) and int32 per-group (``cnt``) names those in ``want`` get
    an array, the others NULL"""
    out = {k: np.empty(tot_pix) for k in pix if k in want}
    out.update({k: np.empty(G) for k in grp if k in want})
    out.update({k: np.empty(G, dtype=np.int32) for k in cnt if k in want})
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    arg = lambda k, ty: out[k].ctypes.data_as(ty) if k in out else None
    return out, [arg(k, dp) for k in pix + grp] + [arg(k, ip) for k in cnt]


def split_records(record, flat, n_pix, steps, pix, grp, cnt):
    """one ``record(step, **fields)`` per group from a call's flat arrays"""
    out, op = [], 0
    for g, (P, st) in enumerate(zip(n_pix, steps)):
        out.append(record(st, **{k: flat[k][op:op + P].copy() for k in pix}, **{k: float(flat[k][g]) for k in grp},
                          **{k: int(flat[k][g]) for k in cnt}))
        op += P
    return out


def pointwise_records(host_call, split, xs, fluxes, noises, chains, n_comp, mode, device, scratch_bytes, steps):
    """the body of ``pointwise_predictive`` / ``pointwise_loo``: ``host_call`` is the module's ``_pred_host`` / ``_loo_host``,
    ``split`` its ``_split``"""
    single = isinstance(chains, np.ndarray)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in ([chains] if single else chains)]
    xs, fluxes, noises = ([v] if single else list(v) for v in (xs, fluxes, noises))
    if not len(xs) == len(fluxes) == len(noises) == len(arrays):
        raise ValueError("one abscissa, one flux and one noise (or None) per chain are required")
    G = len(arrays)
    if G == 0:
        return []
    n_comp, modes, steps = per_group(n_comp, G, int), per_group(mode, G, int), per_group(steps, G, int)
    check_chain_shapes(arrays, n_comp, modes, [int(n is None) for n in noises], [f"free sd = {n is None}" for n in noises])
    flat = host_call(xs, fluxes, noises, arrays, n_comp, modes, steps, int(device), int(scratch_bytes))
    res = split(flat, [len(x) for x in xs], steps)
    return res[0] if single else res


def context_records(call, split, ctx, chain_ptr, n_keep, xs, fluxes, noises, scratch_bytes):
    """the body of ``context_predictive`` / ``context_loo``: ``call`` is the module's ``_call``, ``split`` its ``_split``"""
    ctx.synchronize()                  # the sampler's stream is done with the chain before the default stream reads it
    if isinstance(xs, np.ndarray) and xs.ndim == 1:
        xs, fluxes, noises = [xs], [fluxes], [noises]
    R = len(ctx.ndims)
    if not len(xs) == len(fluxes) == len(noises) == R:
        raise ValueError("one abscissa, one flux and one noise (or None) per region of the context are required")
    ks, modes, sds, bases, ld, n_keep, walkers = context_layout(ctx, chain_ptr, n_keep)
    for sd, n in zip(sds, noises):
        if bool(sd) != (n is None):
            raise ValueError("a region's noise is None exactly when the context samples its sd")
    flat = call(ctx.device, xs, fluxes, noises, ks, modes, sds, bases, True, ld, n_keep, walkers, scratch_bytes)
    return split(flat, [len(x) for x in xs], [1] * R)


def fits_records(pointwise, setter, fits, device, scratch_bytes):
    """the body of ``fits_predictive`` / ``fits_loo``: ``pointwise`` is the module's ``pointwise_*``, ``setter`` the name of
    the method of ``fit.mcmc`` that takes a fit's record"""
    have = fits_with_chain(fits)
    if not have:
        return [], []
    steps = [time_step(f._chain_dev.shape[0], f._chain_dev.shape[1]) for f in have]
    recs = pointwise([f._x for f in have], [f._flux for f in have], [None if f._sample_sd else f.noise for f in have],
                     [f._chain_dev for f in have], [f._n for f in have], [int(f._mode) for f in have], device=device,
                     scratch_bytes=scratch_bytes, steps=steps)
    for f, r in zip(have, recs):
        getattr(f.mcmc, setter)(r)
    return have, recs
