"""Pointwise log predictive density and WAIC of ensemble chains on the GPU: how well the sampled posterior predicts the
data, pixel by pixel (libvamp_pred.so, include/vamp_pred.h; definitions: DESIGN.md "Pointwise predictive density and
WAIC").

    pointwise_predictive(xs, fluxes, noises, chains, n_comp, mode, ...)     host [N, W, D] arrays
    context_predictive(ctx, chain_ptr, n_keep, xs, fluxes, noises)          the device chain HipContext.run_dev wrote
    fits_predictive(fits, ...)                                              the chains of many VPfit objects
    compare(a, b)                                                           elpd difference of two records, paired by pixel

Each call is ONE library call for all the arrays / regions it is given.  Chains and abscissae are in the same units
(a fit's device units: ``fit._chain_dev`` and ``fit._x``).  A ``noise`` of ``None`` means the chain's last dimension
is the free sd, the noise of every pixel.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _pred_lib
from ._sidelib import (MAX_CHAIN_SAMPLES as MAX_SAMPLES, chain_args, check_chain_shapes, context_layout, fits_with_chain, host_layout,
                       per_group, time_step)

HIGH_P_WAIC = 0.4             # a pixel's WAIC is not to be trusted past this p_waic (Vehtari, Gelman & Gabry 2017)

_PIX = ("lppd", "ll_mean", "p_waic_pix")
_GRP = ("elpd_waic", "elpd_se", "p_waic", "lnl_mean")
_CNT = ("n_high", "n_used", "n_bad")
_FLAT = _PIX + _GRP + _CNT


class PredictiveRecord:
    """Pointwise predictive density of one region's ensemble over its ``n_used`` good samples: ``lppd``, ``ll_mean``,
    ``p_waic_pix`` and ``elpd`` = lppd - p_waic_pix [P]; ``elpd_waic``, ``elpd_se``, ``p_waic``, ``lnl_mean`` and ``waic``
    = -2 elpd_waic (floats); ``n_high``: pixels whose p_waic exceeds 0.4; ``step``: every step-th kept sample was read
    (1 unless the chain was longer than the library takes)."""

    __slots__ = _FLAT + ("elpd", "waic", "step")

    def __init__(self, step=1, **fields):
        for k in _FLAT:
            setattr(self, k, fields[k])
        self.elpd = self.lppd - self.p_waic_pix
        self.waic = -2.0 * self.elpd_waic
        self.step = int(step)

    def __repr__(self):
        return (f"PredictiveRecord(P={len(self.lppd)}, elpd_waic={self.elpd_waic!r}, elpd_se={self.elpd_se!r}, p_waic={self.p_waic!r}, "
                f"n_high={self.n_high}, n_used={self.n_used}, n_bad={self.n_bad}, step={self.step})")


def compare(a, b):
    """(difference, standard error) of the expected log predictive density of record ``b`` over record ``a`` on the same
    pixels: sum_p d_p and sqrt(P var_p(d_p)) (P - 1 in the variance), d_p = elpd_p^b - elpd_p^a.  The standard error is
    paired pixel by pixel."""
    if len(a.elpd) != len(b.elpd):
        raise ValueError(f"records of {len(a.elpd)} and {len(b.elpd)} pixels cannot be compared")
    d = np.asarray(b.elpd, dtype=np.float64) - np.asarray(a.elpd, dtype=np.float64)
    P = d.size
    return float(np.sum(d)), (float(np.sqrt(P * np.var(d, ddof=1))) if P > 1 else float("nan"))


def _call(device, xs, fluxes, noises, n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers, scratch_bytes=0, stream=None,
          want=_FLAT):
    """One vamp_pred_pointwise call; returns the flat output arrays by name (group order).  ``want``: the outputs asked
    for (the others are passed as NULL)."""
    lib = _pred_lib.load()
    G = len(bases)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    xs, fluxes = [f64(x) for x in xs], [f64(f) for f in fluxes]
    noises = [None if n is None else f64(n) for n in noises]
    for x, f, n in zip(xs, fluxes, noises):
        if f.shape != x.shape or (n is not None and n.shape != x.shape):
            raise ValueError("flux and noise must have the abscissa's shape")
    tp = int(sum(x.size for x in xs))
    out = {k: np.empty(tp) for k in _PIX if k in want}
    out.update({k: np.empty(G) for k in _GRP if k in want})
    out.update({k: np.empty(G, dtype=np.int32) for k in _CNT if k in want})
    ptrs = lambda arrays: (C.c_void_p * G)(*[None if a is None else a.ctypes.data for a in arrays])
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    arg = lambda k, ty: out[k].ctypes.data_as(ty) if k in out else None
    _pred_lib.check(lib.vamp_pred_pointwise(
        int(device), C.c_void_p(stream or 0), G, ptrs(xs), ptrs(fluxes), ptrs(noises),
        *chain_args([x.size for x in xs], n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers), int(scratch_bytes),
        *[arg(k, dp) for k in _PIX + _GRP], *[arg(k, ip) for k in _CNT]), lib)
    return out


def _pred_host(xs, fluxes, noises, arrays, n_comp, modes, steps, device, scratch_bytes):
    """the library call for contiguous fp64 [N, W, D] host arrays, every ``steps[g]``-th time read in place (tests
    put the numpy restatement here)"""
    bases, ld, n_keep, walkers = host_layout(arrays, steps)
    return _call(device, xs, fluxes, noises, n_comp, modes, [int(n is None) for n in noises], bases, False, ld, n_keep, walkers, scratch_bytes)


def _split(flat, n_pix, steps):
    out, op = [], 0
    for g, (P, st) in enumerate(zip(n_pix, steps)):
        out.append(PredictiveRecord(st, **{k: flat[k][op:op + P].copy() for k in _PIX}, **{k: float(flat[k][g]) for k in _GRP},
                                    **{k: int(flat[k][g]) for k in _CNT}))
        op += P
    return out


def pointwise_predictive(xs, fluxes, noises, chains, n_comp, mode, device=0, scratch_bytes=0, steps=1):
    """Records of one host [N, W, D] chain on the abscissa ``xs`` with the data ``fluxes`` and the noise ``noises``
    (returns one ``PredictiveRecord``) or of a list of chains on lists of those (returns a list), all in one library call.
    A noise of ``None`` means free sd: the chain's last dimension.  ``n_comp``, ``mode`` (0 = Gauss: (A, c, sigma) per
    line, 1 = Voigt: (A, c, L_fwhm, G_fwhm)) and ``steps`` (read every n-th kept sample) are one value for all, or one
    per chain."""
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
    flat = _pred_host(xs, fluxes, noises, arrays, n_comp, modes, steps, int(device), int(scratch_bytes))
    res = _split(flat, [len(x) for x in xs], steps)
    return res[0] if single else res


def context_predictive(ctx, chain_ptr, n_keep, xs, fluxes, noises, scratch_bytes=0):
    """Records of every region of the DEVICE chain ``HipContext.run_dev`` wrote at ``chain_ptr`` ([n_keep, total_theta]
    fp64, e.g. ``tensor.data_ptr()``), read in place, one record per region, from one library call on the context's
    device (default stream, after the context's stream is synchronised).  ``xs``, ``fluxes``, ``noises``: the regions'
    abscissae and data as they were given to ``set_regions``; a region with free sd has the noise ``None``."""
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
    flat = _call(ctx.device, xs, fluxes, noises, ks, modes, sds, bases, True, ld, n_keep, walkers, scratch_bytes)
    return _split(flat, [len(x) for x in xs], [1] * R)


def fits_predictive(fits, device=0, scratch_bytes=0):
    """Records of the chains of many ``VPfit`` objects in ONE library call (device units: ``fit._chain_dev`` on
    ``fit._x``, against ``fit._flux`` with ``fit.noise``, or the chain's sd when ``fit._sample_sd``); each fit's
    ``mcmc.waic()`` cache is filled from it.  A chain of more than MAX_SAMPLES samples is read at the smallest time
    step that fits; the step is each record's ``step``.  Fits without a chain are left out.  Returns (fits scored,
    their records)."""
    have = fits_with_chain(fits)
    if not have:
        return [], []
    steps = [time_step(f._chain_dev.shape[0], f._chain_dev.shape[1]) for f in have]
    recs = pointwise_predictive([f._x for f in have], [f._flux for f in have], [None if f._sample_sd else f.noise for f in have],
                                [f._chain_dev for f in have], [f._n for f in have], [int(f._mode) for f in have], device=device,
                                scratch_bytes=scratch_bytes, steps=steps)
    for f, r in zip(have, recs):
        f.mcmc._set_predictive(r)
    return have, recs
