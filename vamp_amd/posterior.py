"""Posterior summaries of ensemble chains on the GPU: the credible band of the model flux in every pixel and the
equivalent width of every region and line with its credible interval (libvamp_post.so, include/vamp_post.h;
definitions: DESIGN.md "Posterior summaries").

    posterior_summaries(xs, chains, n_comp, mode, ...)      host [N, W, D] arrays
    context_posterior(ctx, chain_ptr, n_keep, xs, ...)      the device chain HipContext.run_dev wrote
    fits_posterior(fits, ...)                               the chains of many VPfit objects

Each call is ONE library call for all the arrays / regions it is given.  Chains and abscissae are in the same
units (a fit's device units: ``fit._chain_dev`` and ``fit._x``); an equivalent width is the sum of the flux
decrement over the pixels times ``pixel_width``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _post_lib
from ._sidelib import (MAX_CHAIN_SAMPLES as MAX_SAMPLES, chain_args, check_chain_shapes, context_layout, fits_with_chain, host_layout,
                       per_group, time_step)

MAX_PROBS = 16
DEFAULT_PROBS = (0.025, 0.16, 0.5, 0.84, 0.975)

_FLAT = ("flux_mean", "flux_sd", "flux_q", "ew_mean", "ew_sd", "ew_q", "comp_ew_mean", "comp_ew_sd", "comp_ew_q", "n_used", "n_bad")


class PosteriorSummary:
    """Summaries of one region's ensemble over its ``n_used`` good samples: ``flux_mean`` / ``flux_sd`` [P],
    ``flux_q`` [Q, P], ``ew_mean`` / ``ew_sd`` (floats), ``ew_q`` [Q], ``comp_ew_mean`` / ``comp_ew_sd`` [K],
    ``comp_ew_q`` [K, Q]; ``probs`` [Q]; ``step``: every step-th kept sample was read (1 unless the chain was longer
    than the library takes)."""

    __slots__ = ("probs",) + _FLAT + ("step",)

    def __init__(self, probs, step=1, **fields):
        self.probs, self.step = probs, int(step)
        for k in _FLAT:
            setattr(self, k, fields[k])

    def __repr__(self):
        return (f"PosteriorSummary(P={len(self.flux_mean)}, K={len(self.comp_ew_mean)}, ew_mean={self.ew_mean!r}, ew_sd={self.ew_sd!r}, "
                f"n_used={self.n_used}, n_bad={self.n_bad}, step={self.step})")


def _probs(probs):
    p = np.ascontiguousarray(np.atleast_1d(probs), dtype=np.float64)
    if p.ndim != 1:
        raise ValueError("probs must be a sequence of numbers")
    return p


def _call(device, xs, n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers, widths, probs, scratch_bytes=0, stream=None):
    """One vamp_post_summaries call; returns the flat output arrays by name (group order)."""
    lib = _post_lib.load()
    G = len(bases)
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
    probs = _probs(probs)
    Q = probs.size
    tp, tk = int(sum(x.size for x in xs)), int(np.sum(n_comp))
    out = {"flux_mean": np.empty(tp), "flux_sd": np.empty(tp), "flux_q": np.empty(tp * Q),
           "ew_mean": np.empty(G), "ew_sd": np.empty(G), "ew_q": np.empty((G, Q)),
           "comp_ew_mean": np.empty(tk), "comp_ew_sd": np.empty(tk), "comp_ew_q": np.empty((tk, Q)),
           "n_used": np.empty(G, dtype=np.int32), "n_bad": np.empty(G, dtype=np.int32)}
    xp = (C.c_void_p * G)(*[x.ctypes.data for x in xs])
    widths = np.ascontiguousarray(widths, dtype=np.float64)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    _post_lib.check(lib.vamp_post_summaries(
        int(device), C.c_void_p(stream or 0), G, xp,
        *chain_args([x.size for x in xs], n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers),
        widths.ctypes.data_as(dp), Q, probs.ctypes.data_as(dp), int(scratch_bytes),
        *[out[k].ctypes.data_as(dp) for k in _FLAT[:9]], out["n_used"].ctypes.data_as(ip), out["n_bad"].ctypes.data_as(ip)), lib)
    return out


def _post_host(xs, arrays, n_comp, modes, sample_sd, widths, probs, steps, device, scratch_bytes):
    """the library call for contiguous fp64 [N, W, D] host arrays, every ``steps[g]``-th time read in place (tests
    put the numpy restatement here)"""
    bases, ld, n_keep, walkers = host_layout(arrays, steps)
    return _call(device, xs, n_comp, modes, sample_sd, bases, False, ld, n_keep, walkers, widths, probs, scratch_bytes)


def _split(flat, n_pix, n_comp, probs, steps):
    Q = probs.size
    out, op, ok = [], 0, 0
    for g, (P, K, st) in enumerate(zip(n_pix, n_comp, steps)):
        out.append(PosteriorSummary(
            probs.copy(), st, flux_mean=flat["flux_mean"][op:op + P].copy(), flux_sd=flat["flux_sd"][op:op + P].copy(),
            flux_q=flat["flux_q"][op * Q:(op + P) * Q].reshape(Q, P).copy(), ew_mean=float(flat["ew_mean"][g]),
            ew_sd=float(flat["ew_sd"][g]), ew_q=flat["ew_q"][g].copy(), comp_ew_mean=flat["comp_ew_mean"][ok:ok + K].copy(),
            comp_ew_sd=flat["comp_ew_sd"][ok:ok + K].copy(), comp_ew_q=flat["comp_ew_q"][ok:ok + K].copy(),
            n_used=int(flat["n_used"][g]), n_bad=int(flat["n_bad"][g])))
        op += P
        ok += K
    return out


def posterior_summaries(xs, chains, n_comp, mode, sample_sd=False, probs=DEFAULT_PROBS, pixel_width=1.0, device=0,
                        scratch_bytes=0, steps=1):
    """Summaries of one host [N, W, D] chain on the abscissa ``xs`` (returns one ``PosteriorSummary``) or of a list
    of chains on a list of abscissae (returns a list), all in one library call.  ``n_comp``, ``mode`` (0 = Gauss:
    (A, c, sigma) per line, 1 = Voigt: (A, c, L_fwhm, G_fwhm)), ``sample_sd``, ``pixel_width`` and ``steps`` (read
    every n-th kept sample) are one value for all, or one per chain."""
    single = isinstance(chains, np.ndarray)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in ([chains] if single else chains)]
    xs = [np.ascontiguousarray(x, dtype=np.float64) for x in ([xs] if single else xs)]
    if len(xs) != len(arrays):
        raise ValueError("one abscissa per chain is required")
    G = len(arrays)
    if G == 0:
        return []
    n_comp, modes, sds = per_group(n_comp, G, int), per_group(mode, G, int), per_group(sample_sd, G, lambda v: int(bool(v)))
    widths, steps = per_group(pixel_width, G, float), per_group(steps, G, int)
    check_chain_shapes(arrays, n_comp, modes, sds, [f"sample_sd = {sd}" for sd in sds])
    probs = _probs(probs)
    flat = _post_host(xs, arrays, n_comp, modes, sds, widths, probs, steps, int(device), int(scratch_bytes))
    res = _split(flat, [x.size for x in xs], n_comp, probs, steps)
    return res[0] if single else res


def context_posterior(ctx, chain_ptr, n_keep, xs, probs=DEFAULT_PROBS, pixel_width=1.0, scratch_bytes=0):
    """Summaries of every region of the DEVICE chain ``HipContext.run_dev`` wrote at ``chain_ptr`` ([n_keep,
    total_theta] fp64, e.g. ``tensor.data_ptr()``), read in place, one record per region, from one library call on the
    context's device (default stream, after the context's stream is synchronised).  ``xs``: the regions' abscissae,
    as they were given to ``set_regions``."""
    ctx.synchronize()                  # the sampler's stream is done with the chain before the default stream reads it
    if isinstance(xs, np.ndarray) and xs.ndim == 1:
        xs = [xs]
    R = len(ctx.ndims)
    if len(xs) != R:
        raise ValueError("one abscissa per region of the context is required")
    ks, modes, sds, bases, ld, n_keep, walkers = context_layout(ctx, chain_ptr, n_keep)
    probs = _probs(probs)
    flat = _call(ctx.device, xs, ks, modes, sds, bases, True, ld, n_keep, walkers, per_group(pixel_width, R, float), probs, scratch_bytes)
    return _split(flat, [len(x) for x in xs], ks, probs, [1] * R)


def fits_posterior(fits, probs=DEFAULT_PROBS, pixel_width=1.0, device=0, scratch_bytes=0):
    """Summaries of the chains of many ``VPfit`` objects in ONE library call (device units: ``fit._chain_dev`` on
    ``fit._x``); each fit's ``mcmc.flux_band()`` / ``mcmc.equivalent_widths()`` cache is filled from it when
    ``pixel_width`` is 1.  A chain of more than MAX_SAMPLES samples is read at the smallest time step that fits; the
    step is each record's ``step``.  Fits without a chain are left out.  Returns (fits summarised, their records)."""
    have = fits_with_chain(fits)
    if not have:
        return [], []
    steps = [time_step(f._chain_dev.shape[0], f._chain_dev.shape[1]) for f in have]
    recs = posterior_summaries([f._x for f in have], [f._chain_dev for f in have], [f._n for f in have], [int(f._mode) for f in have],
                               [bool(f._sample_sd) for f in have], probs=probs, pixel_width=pixel_width, device=device,
                               scratch_bytes=scratch_bytes, steps=steps)
    if np.isscalar(pixel_width) and float(pixel_width) == 1.0:
        for f, r in zip(have, recs):
            f.mcmc._set_posterior(r)
    return have, recs
