"""Convergence diagnostics of ensemble chains on the GPU: integrated autocorrelation time, n_eff and
split-R-hat per parameter (libvamp_diag.so, include/vamp_diag.h; definitions: DESIGN.md "Chain diagnostics").

    chain_diagnostics(chains, thin=1, c=5.0, device=0)   host [N, W, D] arrays
    context_diagnostics(ctx, chain_ptr, n_keep, c=5.0)   the device chain HipContext.run_dev wrote

Each call is ONE library call for all the arrays / regions it is given.  tau is in kept samples;
``record.thin`` converts it to sampler steps (``record.tau * record.thin``).  Both tau and R-hat are
invariant under an affine map of a parameter, so the diagnostics of a fit's device-unit chain are those
of its traces in the caller's units.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _diag_lib
from ._sidelib import fits_with_chain, region_bases

MAX_SAMPLES = 8192            # VAMP_DIAG_MAX_SAMPLES of include/vamp_diag.h


class ChainDiagnostics:
    """Per-parameter diagnostics of one ensemble: arrays of length D."""

    __slots__ = ("tau", "n_eff", "r_hat", "window", "reliable", "thin")

    def __init__(self, tau, n_eff, r_hat, window, reliable, thin=1):
        self.tau, self.n_eff, self.r_hat = tau, n_eff, r_hat
        self.window, self.reliable, self.thin = window, reliable, int(thin)

    def __repr__(self):
        return (f"ChainDiagnostics(tau={self.tau!r}, n_eff={self.n_eff!r}, r_hat={self.r_hat!r}, window={self.window!r}, "
                f"reliable={self.reliable!r}, thin={self.thin})")


def _call(device, bases, is_device, ld, n_keep, walkers, ndim, c, stream=None):
    """One vamp_diag_chains call; returns flat (tau, n_eff, r_hat, window, reliable) over sum(ndim)."""
    lib = _diag_lib.load()
    G = len(bases)
    total = int(np.sum(ndim))
    tau, n_eff, r_hat = np.empty(total), np.empty(total), np.empty(total)
    window = np.empty(total, dtype=np.int32)
    reliable = np.empty(total, dtype=np.uint8)
    ptrs = (C.c_void_p * G)(*[int(b) for b in bases])
    ld = np.ascontiguousarray(ld, dtype=np.int64)
    n_keep, walkers, ndim = (np.ascontiguousarray(a, dtype=np.int32) for a in (n_keep, walkers, ndim))
    i32 = C.POINTER(C.c_int32)
    dp = C.POINTER(C.c_double)
    _diag_lib.check(lib.vamp_diag_chains(
        int(device), C.c_void_p(stream or 0), G, ptrs, int(bool(is_device)), ld.ctypes.data_as(C.POINTER(C.c_int64)),
        n_keep.ctypes.data_as(i32), walkers.ctypes.data_as(i32), ndim.ctypes.data_as(i32), float(c),
        tau.ctypes.data_as(dp), n_eff.ctypes.data_as(dp), r_hat.ctypes.data_as(dp), window.ctypes.data_as(i32),
        reliable.ctypes.data_as(C.POINTER(C.c_uint8))), lib)
    return tau, n_eff, r_hat, window, reliable.astype(bool)


def _diag_host(arrays, c, device):
    """the library call for a list of contiguous fp64 [N, W, D] host arrays (tests put the numpy restatement here)"""
    return _call(device, [a.ctypes.data for a in arrays], False, [a.shape[1] * a.shape[2] for a in arrays],
                 [a.shape[0] for a in arrays], [a.shape[1] for a in arrays], [a.shape[2] for a in arrays], c)


def _split(flat, ndims, thins):
    out, o = [], 0
    for d, th in zip(ndims, thins):
        out.append(ChainDiagnostics(*(a[o:o + d].copy() for a in flat), thin=th))
        o += d
    return out


def chain_diagnostics(chains, thin=1, c=5.0, device=0):
    """Diagnostics of one host [N, W, D] chain (returns one ``ChainDiagnostics``) or of a list of them (returns a
    list), all in one library call.  ``thin``: the sampler steps per kept sample (an int, or one per chain)."""
    single = isinstance(chains, np.ndarray)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in ([chains] if single else chains)]
    for a in arrays:
        if a.ndim != 3:
            raise ValueError("every chain must be an [N, W, D] array")
    thins = [int(thin)] * len(arrays) if np.isscalar(thin) else [int(t) for t in thin]
    if len(thins) != len(arrays):
        raise ValueError("one thin per chain is required")
    if not arrays:
        return []
    res = _split(_diag_host(arrays, float(c), int(device)), [a.shape[2] for a in arrays], thins)
    return res[0] if single else res


def context_diagnostics(ctx, chain_ptr, n_keep, c=5.0, thin=1):
    """Diagnostics of every region of the DEVICE chain ``HipContext.run_dev`` wrote at ``chain_ptr``
    ([n_keep, total_theta] fp64, e.g. ``tensor.data_ptr()``), one record per region, from one library call on the
    context's device (default stream, after the context's stream is synchronised)."""
    ctx.synchronize()                  # the sampler's stream is done with the chain before the default stream reads it
    W, ndims = int(ctx.W), list(ctx.ndims)
    R = len(ndims)
    flat = _call(ctx.device, region_bases(ctx, chain_ptr), True, [ctx.total_theta] * R, [int(n_keep)] * R, [W] * R, ndims, float(c))
    return _split(flat, ndims, [int(thin)] * R)


def fits_diagnostics(fits, c=5.0, device=0):
    """Diagnostics of the chains of many ``VPfit`` objects in ONE library call; each fit's ``mcmc.diagnostics()``
    cache is filled from it.  Fits without a chain are left out; so are chains of more than MAX_SAMPLES kept samples,
    which the library rejects (a long run, e.g. ``--iterations 10000 --thin 1``, must still get its perf record).
    Returns (records of the fits diagnosed, number of fits left out for their length)."""
    have = fits_with_chain(fits)
    ok = [f for f in have if f._chain_dev.shape[0] <= MAX_SAMPLES]
    skipped = len(have) - len(ok)
    if not ok:
        return [], skipped
    recs = chain_diagnostics([f._chain_dev for f in ok], thin=[f.mcmc._thin for f in ok], c=c, device=device)
    for f, r in zip(ok, recs):
        f.mcmc._set_diagnostics(r)
    return recs, skipped


def summary(records):
    """The spectrum-level numbers of do_vamp's perf record from per-region records: the smallest n_eff, the share of
    regions whose smallest n_eff is below 50, the largest R-hat, the share of regions with an unreliable tau (shares of
    the regions diagnosed).  A number that is not finite-or-infinite (NaN) is reported as None; so is every field when
    no region was diagnosed."""
    def num(v):
        return None if v is None or np.isnan(v) else float(v)
    if not records:
        return {"min_n_eff": None, "frac_regions_n_eff_below_50": None, "max_r_hat": None, "frac_regions_unreliable_tau": None}
    with np.errstate(invalid="ignore"):
        reg_min = np.array([np.nanmin(r.n_eff) if np.any(~np.isnan(r.n_eff)) else np.nan for r in records])
        reg_rhat = np.array([np.nanmax(r.r_hat) if np.any(~np.isnan(r.r_hat)) else np.nan for r in records])
    return {"min_n_eff": num(np.nanmin(reg_min)) if np.any(~np.isnan(reg_min)) else None,
            "frac_regions_n_eff_below_50": float(np.mean(reg_min < 50.0)),
            "max_r_hat": num(np.nanmax(reg_rhat)) if np.any(~np.isnan(reg_rhat)) else None,
            "frac_regions_unreliable_tau": float(np.mean([not bool(np.all(r.reliable)) for r in records]))}
