"""Fisher-matrix errors at a point on the GPU: the gradient of the log-posterior, the Gauss-Newton information matrix
and its inverse from the analytic Jacobian of the model flux (libvamp_fisher.so, include/vamp_fisher.h; definitions:
DESIGN.md section 15).  At the MAP the inverse is the covariance a line fitter reports; it needs no chain.

    fisher_points(xs, fluxes, noises, thetas, n_comp, mode, ...)      host points [D] or [n, D]
    context_fisher(ctx, theta_ptr, xs, fluxes, noises, ...)           device points, one row of all regions' vectors each
    fits_fisher(fits, ...)                                            many VPfit objects at their current point

Each call is ONE library call for all the regions and points it is given.  Points and abscissae are in the same units
(a fit's device units: ``fit._theta_dev`` on ``fit._x``); ``fits_fisher`` hands back records in the caller's units.
A ``noise`` of ``None`` means the point's last entry is the free sd, the noise of every pixel.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _fisher_lib
from ._sidelib import Q_OF_MODE, per_group

MAX_COMPONENTS = 16           # VAMP_FISHER_MAX_COMPONENTS of include/vamp_fisher.h
MAX_MATRIX_DOUBLES = 1 << 26  # VAMP_FISHER_MAX_MATRIX_DOUBLES

_VEC = ("grad", "sigma")
_MAT = ("info", "cov")
_PT = ("logdet", "chi2")
_ALL = _VEC + _MAT + _PT + ("status", "jac")


class FisherRecord:
    """One point's ``grad`` [D], ``info`` and ``cov`` [D, D], ``sigma`` [D] = sqrt(diag cov), ``corr`` [D, D], ``logdet``
    = ln det info, ``chi2``, ``status`` (0 ok; 1 info not positive definite: cov, sigma, logdet NaN; 2 bad point:
    everything NaN), ``jac`` [P, D] when it was asked for (else None) and ``names`` (the fit's parameter names when the
    record was made from a fit, else None)."""

    __slots__ = ("grad", "info", "cov", "sigma", "corr", "logdet", "chi2", "status", "jac", "names")

    def __init__(self, grad, info, cov, sigma, logdet, chi2, status, jac=None, names=None):
        self.grad, self.info, self.cov, self.sigma = grad, info, cov, sigma
        self.logdet, self.chi2, self.status, self.jac = float(logdet), float(chi2), int(status), jac
        self.names = None if names is None else list(names)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.corr = cov / np.outer(sigma, sigma)

    def to_units(self, scale, names=None):
        """the record of the same point in units theta' = theta * scale + shift: cov' = diag(scale) cov diag(scale),
        grad' = grad / scale, info' = info / (scale x scale), logdet' = logdet - 2 sum ln |scale|, jac' = jac / scale"""
        s = np.asarray(scale, dtype=np.float64)
        if s.shape != self.grad.shape:
            raise ValueError(f"{s.size} scales for a record of {self.grad.size} parameters")
        ss = np.outer(s, s)
        return FisherRecord(self.grad / s, self.info / ss, self.cov * ss, self.sigma * np.abs(s),
                            self.logdet - 2.0 * float(np.sum(np.log(np.abs(s)))), self.chi2, self.status,
                            None if self.jac is None else self.jac / s, self.names if names is None else names)

    def __repr__(self):
        return f"FisherRecord(D={self.grad.size}, status={self.status}, chi2={self.chi2!r}, logdet={self.logdet!r})"


def _call(device, xs, fluxes, noises, n_comp, modes, sample_sd, bases, is_device, ld, n_points, with_prior=True, stream=None,
          want=_ALL):
    """One vamp_fisher_points call; returns the flat output arrays by name (group order).  ``want``: the outputs asked
    for (the others are passed as NULL)."""
    lib = _fisher_lib.load()
    G = len(bases)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    xs, fluxes = [f64(x) for x in xs], [f64(f) for f in fluxes]
    noises = [None if n is None else f64(n) for n in noises]
    for x, f, n in zip(xs, fluxes, noises):
        if x.ndim != 1 or f.shape != x.shape or (n is not None and n.shape != x.shape):
            raise ValueError("flux and noise must have the abscissa's shape")
    dims = [Q_OF_MODE.get(m, 3) * k + sd for m, k, sd in zip(modes, n_comp, sample_sd)]
    n_vec = int(sum(n * d for n, d in zip(n_points, dims)))
    n_mat = int(sum(n * d * d for n, d in zip(n_points, dims)))
    n_pt = int(sum(n_points))
    n_jac = int(sum(n * d * x.size for n, d, x in zip(n_points, dims, xs)))
    sizes = {**{k: n_vec for k in _VEC}, **{k: n_mat for k in _MAT}, **{k: n_pt for k in _PT}, "jac": n_jac}
    out = {k: np.empty(sizes[k]) for k in _VEC + _MAT + _PT + ("jac",) if k in want}
    if "status" in want:
        out["status"] = np.empty(n_pt, dtype=np.int32)
    ptrs = lambda arrays: (C.c_void_p * G)(*[None if a is None else a.ctypes.data for a in arrays])
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ip)
    arg = lambda k, ty: out[k].ctypes.data_as(ty) if k in out else None
    _fisher_lib.check(lib.vamp_fisher_points(
        int(device), C.c_void_p(stream or 0), G, ptrs(xs), ptrs(fluxes), ptrs(noises), i32([x.size for x in xs]), i32(n_comp),
        i32(modes), i32(sample_sd), (C.c_void_p * G)(*[int(b) for b in bases]), int(bool(is_device)),
        np.ascontiguousarray(ld, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64)), i32(n_points), int(bool(with_prior)),
        arg("grad", dp), arg("info", dp), arg("cov", dp), arg("sigma", dp), arg("logdet", dp), arg("chi2", dp), arg("status", ip),
        arg("jac", dp)), lib)
    return out


def _split(flat, dims, n_pix, n_points, jac):
    """the flat outputs of ``_call`` (everything asked for) as one list of records per group"""
    out, ov, om, op, oj = [], 0, 0, 0, 0
    for D, P, n in zip(dims, n_pix, n_points):
        recs = []
        for _ in range(n):
            recs.append(FisherRecord(flat["grad"][ov:ov + D].copy(), flat["info"][om:om + D * D].reshape(D, D).copy(),
                                     flat["cov"][om:om + D * D].reshape(D, D).copy(), flat["sigma"][ov:ov + D].copy(),
                                     flat["logdet"][op], flat["chi2"][op], flat["status"][op],
                                     flat["jac"][oj:oj + P * D].reshape(P, D).copy() if jac else None))
            ov, om, op = ov + D, om + D * D, op + 1
            oj += P * D if jac else 0
        out.append(recs)
    return out


def _want(jac):
    return _ALL if jac else tuple(k for k in _ALL if k != "jac")


def fisher_points(xs, fluxes, noises, thetas, n_comp, mode, with_prior=True, device=0, jac=False):
    """Records at host points of one region -- ``xs`` a 1-D abscissa, ``thetas`` one point [D] (returns a record) or
    [n, D] (returns a list) -- or of a list of regions with one such entry each (returns a list of those), all in one
    library call.  A noise of ``None`` means free sd: the point's last entry.  ``n_comp`` and ``mode`` (0 = Gauss: (A, c,
    sigma) per line, 1 = Voigt: (A, c, L_fwhm, G_fwhm)) are one value for all, or one per region.  ``with_prior``:
    include the curvature and slope of the amplitudes' x e^-x prior.  ``jac``: also return the Jacobian [P, D]."""
    single = isinstance(xs, np.ndarray) and xs.ndim == 1
    if single:
        xs, fluxes, noises, thetas = [xs], [fluxes], [noises], [thetas]
    xs, fluxes, noises, thetas = list(xs), list(fluxes), list(noises), list(thetas)
    if not len(xs) == len(fluxes) == len(noises) == len(thetas):
        raise ValueError("one abscissa, one flux, one noise (or None) and one set of points per region are required")
    G = len(xs)
    if G == 0:
        return []
    n_comp, modes = per_group(n_comp, G, int), per_group(mode, G, int)
    sds = [int(n is None) for n in noises]
    arrays = [np.ascontiguousarray(t, dtype=np.float64) for t in thetas]
    one = [a.ndim == 1 for a in arrays]
    arrays = [np.atleast_2d(a) for a in arrays]
    for a, k, m, sd in zip(arrays, n_comp, modes, sds):
        if a.ndim != 2 or a.shape[0] < 1:
            raise ValueError("the points of a region must be a [D] or a non-empty [n, D] array")
        if m not in Q_OF_MODE:
            raise ValueError(f"mode {m} is not supported (0 = Gauss, 1 = Voigt)")
        if not 1 <= k <= MAX_COMPONENTS:
            raise ValueError(f"n_comp = {k} is outside 1 .. {MAX_COMPONENTS}")
        if a.shape[1] != Q_OF_MODE[m] * k + sd:
            raise ValueError(f"a point of {a.shape[1]} parameters does not hold {k} lines of mode {m} (free sd = {bool(sd)})")
    dims, n_points = [a.shape[1] for a in arrays], [a.shape[0] for a in arrays]
    if sum(n * d * d for n, d in zip(n_points, dims)) > MAX_MATRIX_DOUBLES:
        raise ValueError(f"more than {MAX_MATRIX_DOUBLES} matrix entries in one call: split it")
    flat = _call(int(device), xs, fluxes, noises, n_comp, modes, sds, [a.ctypes.data for a in arrays], False, dims, n_points,
                 with_prior=with_prior, want=_want(jac))
    recs = _split(flat, dims, [len(x) for x in xs], n_points, jac)
    recs = [r[0] if o else r for r, o in zip(recs, one)]
    return recs[0] if single else recs


def context_fisher(ctx, theta_ptr, xs, fluxes, noises, n_points=1, with_prior=True, jac=False, stream=None):
    """Records at DEVICE points of every region of a context: ``theta_ptr`` addresses fp64 [n_points, sum of the regions'
    D], a row holding the regions' vectors side by side (e.g. ``tensor.data_ptr()``), read in place by one library call
    on the context's device (after the context's stream is synchronised).  ``xs``, ``fluxes``, ``noises``: the regions'
    abscissae and data as they were given to ``set_regions``; a region with free sd has the noise ``None``.  Returns
    one list of ``n_points`` records per region."""
    ctx.synchronize()
    if isinstance(xs, np.ndarray) and xs.ndim == 1:
        xs, fluxes, noises = [xs], [fluxes], [noises]
    R, mode = len(ctx.ndims), int(ctx.mode)
    if not len(xs) == len(fluxes) == len(noises) == R:
        raise ValueError("one abscissa, one flux and one noise (or None) per region of the context are required")
    if mode not in Q_OF_MODE:
        raise ValueError(f"mode {mode} is not supported (0 = Gauss, 1 = Voigt)")
    ks = [int(k) for k in ctx.n_comp]
    dims = [int(d) for d in ctx.ndims]
    sds = [d - Q_OF_MODE[mode] * k for d, k in zip(dims, ks)]
    for sd, n in zip(sds, noises):
        if bool(sd) != (n is None):
            raise ValueError("a region's noise is None exactly when the context samples its sd")
    offs = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
    bases = [int(theta_ptr) + 8 * int(o) for o in offs[:-1]]
    n_points = int(n_points)
    flat = _call(ctx.device, xs, fluxes, noises, ks, [mode] * R, sds, bases, True, [int(offs[-1])] * R, [n_points] * R,
                 with_prior=with_prior, stream=stream, want=_want(jac))
    return _split(flat, dims, [len(x) for x in xs], [n_points] * R, jac)


def fits_fisher(fits, with_prior=True, device=0, jac=False):
    """Records of many ``VPfit`` objects at their current point (``fit._theta_dev``: the MAP after ``map_estimate``) in
    ONE library call, converted to the caller's units with the affine map of ``VPfit._to_caller`` and named with the
    fits' parameter names; each fit's ``fisher()`` cache is filled.  Returns the records, one per fit."""
    fits = list(fits)
    if not fits:
        return []
    recs = fisher_points([f._x for f in fits], [f._flux for f in fits], [None if f._sample_sd else f.noise for f in fits],
                         [np.asarray(f._theta_dev, dtype=np.float64) for f in fits], [f._n for f in fits], [int(f._mode) for f in fits],
                         with_prior=with_prior, device=device, jac=jac)
    out = []
    for f, r in zip(fits, recs):
        rec = r.to_units(f._scale, names=f._names)
        f._set_fisher(rec, with_prior)
        out.append(rec)
    return out
