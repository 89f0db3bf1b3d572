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
from ._sidelib import (MAX_CHAIN_SAMPLES as MAX_SAMPLES, chain_args, context_records, data_args, fits_records, host_layout, outputs,
                       pointer_array, pointwise_records, split_records, time_step)

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
    xs, fluxes, noises = data_args(xs, fluxes, noises)
    out, args = outputs(G, int(sum(x.size for x in xs)), want, _PIX, _GRP, _CNT)
    _pred_lib.check(lib.vamp_pred_pointwise(
        int(device), C.c_void_p(stream or 0), G, pointer_array(xs), pointer_array(fluxes), pointer_array(noises),
        *chain_args([x.size for x in xs], n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers), int(scratch_bytes), *args), lib)
    return out


def _pred_host(xs, fluxes, noises, arrays, n_comp, modes, steps, device, scratch_bytes):
    """the library call for contiguous fp64 [N, W, D] host arrays, every ``steps[g]``-th time read in place (tests
    put the numpy restatement here)"""
    bases, ld, n_keep, walkers = host_layout(arrays, steps)
    return _call(device, xs, fluxes, noises, n_comp, modes, [int(n is None) for n in noises], bases, False, ld, n_keep, walkers, scratch_bytes)


def _split(flat, n_pix, steps):
    return split_records(PredictiveRecord, flat, n_pix, steps, _PIX, _GRP, _CNT)


def pointwise_predictive(xs, fluxes, noises, chains, n_comp, mode, device=0, scratch_bytes=0, steps=1):
    """Records of one host [N, W, D] chain on the abscissa ``xs`` with the data ``fluxes`` and the noise ``noises``
    (returns one ``PredictiveRecord``) or of a list of chains on lists of those (returns a list), all in one library call.
    A noise of ``None`` means free sd: the chain's last dimension.  ``n_comp``, ``mode`` (0 = Gauss: (A, c, sigma) per
    line, 1 = Voigt: (A, c, L_fwhm, G_fwhm)) and ``steps`` (read every n-th kept sample) are one value for all, or one
    per chain."""
    return pointwise_records(_pred_host, _split, xs, fluxes, noises, chains, n_comp, mode, device, scratch_bytes, steps)


def context_predictive(ctx, chain_ptr, n_keep, xs, fluxes, noises, scratch_bytes=0):
    """Records of every region of the DEVICE chain ``HipContext.run_dev`` wrote at ``chain_ptr`` ([n_keep, total_theta]
    fp64, e.g. ``tensor.data_ptr()``), read in place, one record per region, from one library call on the context's
    device (default stream, after the context's stream is synchronised).  ``xs``, ``fluxes``, ``noises``: the regions'
    abscissae and data as they were given to ``set_regions``; a region with free sd has the noise ``None``."""
    return context_records(_call, _split, ctx, chain_ptr, n_keep, xs, fluxes, noises, scratch_bytes)


def fits_predictive(fits, device=0, scratch_bytes=0):
    """Records of the chains of many ``VPfit`` objects in ONE library call (device units: ``fit._chain_dev`` on
    ``fit._x``, against ``fit._flux`` with ``fit.noise``, or the chain's sd when ``fit._sample_sd``); each fit's
    ``mcmc.waic()`` cache is filled from it.  A chain of more than MAX_SAMPLES samples is read at the smallest time
    step that fits; the step is each record's ``step``.  Fits without a chain are left out.  Returns (fits scored,
    their records)."""
    return fits_records(pointwise_predictive, "_set_predictive", fits, device, scratch_bytes)
