"""PSIS-LOO of ensemble chains on the GPU: the Pareto-smoothed importance-sampling leave-one-out predictive density of
every pixel, valid where a pixel's WAIC is not (``PredictiveRecord.n_high``), with the Pareto shape khat that says
when not even LOO can be trusted (libvamp_loo.so, include/vamp_loo.h; definitions: DESIGN.md "PSIS-LOO: leave-one-out
predictive density per pixel").

    pointwise_loo(xs, fluxes, noises, chains, n_comp, mode, ...)     host [N, W, D] arrays
    context_loo(ctx, chain_ptr, n_keep, xs, fluxes, noises)          the device chain HipContext.run_dev wrote
    fits_loo(fits, ...)                                              the chains of many VPfit objects
    loo_from_loglik(ll, skip=None, ...)                              log-likelihood matrices [S, P] the caller already has
    predictive.compare(a, b)                                         elpd difference of two records, paired by pixel

Each call is ONE library call for all the arrays / regions it is given.  Chains and abscissae are in the same units
(a fit's device units: ``fit._chain_dev`` and ``fit._x``).  A ``noise`` of ``None`` means the chain's last dimension
is the free sd, the noise of every pixel.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _loo_lib
from ._sidelib import (MAX_CHAIN_SAMPLES as MAX_SAMPLES, chain_args, context_records, data_args, fits_records, host_layout, outputs,
                       pointer_array, pointwise_records, split_records, time_step)

HIGH_KHAT = 0.7               # a pixel's PSIS-LOO is not to be trusted past this khat (Vehtari, Gelman & Gabry 2017)

_PIX = ("elpd_loo_pix", "p_loo_pix", "khat", "lppd")
_GRP = ("elpd_loo", "elpd_loo_se", "p_loo")
_CNT = ("n_high_k", "n_used", "n_bad")
_FLAT = _PIX + _GRP + _CNT


class LooRecord:
    """PSIS-LOO of one region's ensemble over its ``n_used`` good samples: ``elpd_loo_pix`` (alias ``elpd``, what
    ``predictive.compare`` pairs), ``p_loo_pix`` = lppd - elpd_loo_pix, ``khat`` and ``lppd`` [P]; ``elpd_loo``,
    ``elpd_loo_se``, ``p_loo`` and ``looic`` = -2 elpd_loo (floats); ``n_high_k``: pixels whose khat exceeds 0.7;
    ``step``: every step-th kept sample was read (1 unless the chain was longer than the library takes)."""

    __slots__ = _FLAT + ("looic", "step")

    def __init__(self, step=1, **fields):
        for k in _FLAT:
            setattr(self, k, fields[k])
        self.looic = -2.0 * self.elpd_loo
        self.step = int(step)

    @property
    def elpd(self):
        return self.elpd_loo_pix

    def __repr__(self):
        return (f"LooRecord(P={len(self.lppd)}, elpd_loo={self.elpd_loo!r}, elpd_loo_se={self.elpd_loo_se!r}, p_loo={self.p_loo!r}, "
                f"n_high_k={self.n_high_k}, n_used={self.n_used}, n_bad={self.n_bad}, step={self.step})")


def _call(device, xs, fluxes, noises, n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers, scratch_bytes=0, stream=None,
          want=_FLAT):
    """One vamp_loo_pointwise call; returns the flat output arrays by name (group order).  ``want``: the outputs asked
    for (the others are passed as NULL); with ``"ll"`` among them the result also holds ``ll``: per group the [S, P]
    log-likelihood matrix the call used (rows of bad samples NaN)."""
    lib = _loo_lib.load()
    G = len(bases)
    xs, fluxes, noises = data_args(xs, fluxes, noises)
    out, args = outputs(G, int(sum(x.size for x in xs)), want, _PIX, _GRP, _CNT)
    ll = None
    if "ll" in want:
        ll = [np.empty((int(n) * int(w), x.size)) for n, w, x in zip(n_keep, walkers, xs)]
    _loo_lib.check(lib.vamp_loo_pointwise(
        int(device), C.c_void_p(stream or 0), G, pointer_array(xs), pointer_array(fluxes), pointer_array(noises),
        *chain_args([x.size for x in xs], n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers), int(scratch_bytes),
        *args, None if ll is None else pointer_array(ll)), lib)
    if ll is not None:
        out["ll"] = ll
    return out


def _call_loglik(device, lls, n_samples, n_pix, skips=None, is_device=False, scratch_bytes=0, stream=None, want=_FLAT):
    """One vamp_loo_from_loglik call on the matrices at the addresses ``lls`` ([n_samples[g], n_pix[g]] fp64,
    sample-major, host or device according to ``is_device``); ``skips``: None, or per group None or a uint8 [S] array."""
    lib = _loo_lib.load()
    G = len(lls)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    out, args = outputs(G, int(sum(int(p) for p in n_pix)), want, _PIX, _GRP, _CNT)
    skip_arg = None
    if skips is not None:
        skips = [None if s is None else np.ascontiguousarray(s, dtype=np.uint8) for s in skips]
        for s, n in zip(skips, n_samples):
            if s is not None and s.shape != (int(n),):
                raise ValueError("skip must hold one byte per sample")
        skip_arg = (C.c_void_p * G)(*[None if s is None else s.ctypes.data for s in skips])
    _loo_lib.check(lib.vamp_loo_from_loglik(int(device), C.c_void_p(stream or 0), G, (C.c_void_p * G)(*[int(p) for p in lls]),
                                            int(bool(is_device)), i32(n_samples), i32(n_pix), skip_arg, int(scratch_bytes), *args), lib)
    return out


def _loo_host(xs, fluxes, noises, arrays, n_comp, modes, steps, device, scratch_bytes):
    """the library call for contiguous fp64 [N, W, D] host arrays, every ``steps[g]``-th time read in place (tests
    put the numpy restatement here)"""
    bases, ld, n_keep, walkers = host_layout(arrays, steps)
    return _call(device, xs, fluxes, noises, n_comp, modes, [int(n is None) for n in noises], bases, False, ld, n_keep, walkers, scratch_bytes)


def _split(flat, n_pix, steps):
    return split_records(LooRecord, flat, n_pix, steps, _PIX, _GRP, _CNT)


def pointwise_loo(xs, fluxes, noises, chains, n_comp, mode, device=0, scratch_bytes=0, steps=1):
    """Records of one host [N, W, D] chain on the abscissa ``xs`` with the data ``fluxes`` and the noise ``noises``
    (returns one ``LooRecord``) or of a list of chains on lists of those (returns a list), all in one library call.
    The arguments are those of ``predictive.pointwise_predictive``."""
    return pointwise_records(_loo_host, _split, xs, fluxes, noises, chains, n_comp, mode, device, scratch_bytes, steps)


def context_loo(ctx, chain_ptr, n_keep, xs, fluxes, noises, scratch_bytes=0):
    """Records of every region of the DEVICE chain ``HipContext.run_dev`` wrote at ``chain_ptr`` ([n_keep, total_theta]
    fp64), read in place, one record per region, from one library call on the context's device (default stream, after
    the context's stream is synchronised).  The arguments are those of ``predictive.context_predictive``."""
    return context_records(_call, _split, ctx, chain_ptr, n_keep, xs, fluxes, noises, scratch_bytes)


def fits_loo(fits, device=0, scratch_bytes=0):
    """Records of the chains of many ``VPfit`` objects in ONE library call (as ``predictive.fits_predictive``); each
    fit's ``mcmc.loo()`` cache is filled from it.  A chain of more than MAX_SAMPLES samples is read at the smallest
    time step that fits; the step is each record's ``step``.  Fits without a chain are left out.  Returns (fits
    scored, their records)."""
    return fits_records(pointwise_loo, "_set_loo", fits, device, scratch_bytes)


def loo_from_loglik(ll, skip=None, device=0, scratch_bytes=0):
    """PSIS-LOO of log-likelihood matrices the caller already has (arviz's ``log_likelihood``): ``ll`` is one [S, P]
    matrix (returns one ``LooRecord``) or a list of them (returns a list), each a numpy array (host) or a contiguous
    fp64 device tensor with ``data_ptr()`` and ``shape``, all of one kind; ``skip``: per matrix None or S flags, 1 =
    leave the sample out.  One library call."""
    single = isinstance(ll, np.ndarray) or hasattr(ll, "data_ptr")
    mats = [ll] if single else list(ll)
    skips = None if skip is None else ([skip] if single else list(skip))
    if not mats:
        return []
    on_device = [hasattr(m, "data_ptr") for m in mats]
    if any(on_device) != all(on_device):
        raise ValueError("the matrices must all be host arrays or all device tensors")
    if on_device[0]:
        for m in mats:
            if str(m.dtype) != "torch.float64" or not m.is_contiguous():
                raise ValueError("a device matrix must be a contiguous fp64 tensor")
        ptrs = [m.data_ptr() for m in mats]
    else:
        mats = [np.ascontiguousarray(m, dtype=np.float64) for m in mats]
        ptrs = [m.ctypes.data for m in mats]
    if any(len(m.shape) != 2 for m in mats):
        raise ValueError("every log-likelihood matrix must be [S, P]")
    flat = _call_loglik(device, ptrs, [m.shape[0] for m in mats], [m.shape[1] for m in mats], skips, on_device[0], scratch_bytes)
    res = _split(flat, [m.shape[1] for m in mats], [1] * len(mats))
    return res[0] if single else res
