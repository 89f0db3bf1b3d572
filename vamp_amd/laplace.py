"""Laplace importance sampling on the GPU: ln Z with a standard error and the posterior's mean, standard deviations and
covariance from independent draws of a Gaussian proposal around a point, weighted by the exact posterior and
Pareto-smoothed (libvamp_laplace.so, include/vamp_laplace.h; definitions: DESIGN.md section 16).  It needs no chain;
``khat`` says per region whether the proposal covers the posterior well enough to trust the rest (<= 0.7).

    laplace_points(xs, fluxes, noises, centres, covs, n_comp, mode, ...)      host centres and covariances
    fits_laplace(fits, ...)                                                   many VPfit objects at their current point

Each call is ONE library call for all the regions it is given.  Centres, covariances and abscissae are in the same
units (a fit's device units: ``fit._theta_dev`` on ``fit._x``); ``fits_laplace`` hands back records in the caller's units.
A ``noise`` of ``None`` means the centre's last entry is the free sd, the noise of every pixel.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _laplace_lib
from ._sidelib import Q_OF_MODE, per_group

MAX_COMPONENTS, MAX_SAMPLES = 16, 16384       # of include/vamp_laplace.h
DEFAULT_SEED = 20110101
METRICS = ("fisher", "regularised", "chain")
HIGH_KHAT = 0.7                               # Vehtari et al.: above it the estimates are not to be trusted

_GRP = ("lnZ", "lnZ_se", "lnZ_psis", "khat", "ess", "lnp_centre")
_CNT = ("n_out", "status")
_VEC = ("mean", "sd")
_SAMPLE_MAT = ("theta", "z")
_SAMPLE_VEC = ("lnp", "lnq", "lw")
_SAMPLES = _SAMPLE_MAT + _SAMPLE_VEC
_DP, _IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class LaplaceRecord:
    """One region's ``lnZ`` (plain importance sampling) with ``lnZ_se``, ``lnZ_psis`` (from the smoothed weights),
    ``lnZ_laplace`` (the plain Laplace estimate ln p(centre) + (D / 2) ln 2 pi - logdet / 2, logdet = ln det of the
    information), ``khat``, ``ess``, ``n_out`` (draws outside the prior or without a finite ln L), ``status`` (0 ok; 1 no
    proposal; 2 the centre is rejected by the target: everything NaN), ``mean`` / ``sd`` [D], ``cov`` [D, D],
    ``lnp_centre``, ``n_samples``, ``inflate``, ``names`` (the fit's parameter names when the record was made from a fit,
    else None), ``metric`` (what ``fits_laplace`` took the proposal from, else None) with ``n_low`` / ``n_high`` (the
    directions a regularised metric repaired; None with the Fisher metric) and -- when asked for, else None -- the draws ``theta`` / ``z`` [S, D] and ``lnp`` / ``lnq`` / ``lw`` [S]."""

    __slots__ = _GRP + _CNT + _VEC + ("cov", "lnZ_laplace", "n_samples", "inflate", "names", "metric", "n_low", "n_high") + _SAMPLES

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields.get(k))

    @property
    def ok(self):
        """status 0 and khat <= 0.7"""
        return self.status == 0 and bool(self.khat <= HIGH_KHAT)

    def to_units(self, scale, shift=None, names=None):
        """the record of the same posterior in units theta' = theta * scale + shift: mean' = mean * scale + shift, sd' = sd
        |scale|, cov' = diag(scale) cov diag(scale), theta' likewise; ln Z, khat, ess and the weights do not change (the
        evidence is that of the model as the library's priors state it)"""
        s = np.asarray(scale, dtype=np.float64)
        if s.shape != self.mean.shape:
            raise ValueError(f"{s.size} scales for a record of {self.mean.size} parameters")
        t = np.zeros_like(s) if shift is None else np.asarray(shift, dtype=np.float64)
        f = {k: getattr(self, k) for k in self.__slots__}
        f.update(mean=self.mean * s + t, sd=self.sd * np.abs(s), cov=self.cov * np.outer(s, s),
                 theta=None if self.theta is None else self.theta * s + t, names=self.names if names is None else list(names))
        return LaplaceRecord(**f)

    def __repr__(self):
        return (f"LaplaceRecord(D={self.mean.size}, status={self.status}, lnZ={self.lnZ!r}, lnZ_se={self.lnZ_se!r}, khat={self.khat!r}, "
                f"ess={self.ess!r}, n_out={self.n_out})")


def _call(device, xs, fluxes, noises, n_comp, modes, sample_sd, bounds, region_ids, centres, chols, n_samples, seed, want=_SAMPLES,
          stream=None, device_ptrs=None, skip=()):
    """One vamp_laplace_points call; returns the flat per-group arrays by name (group order) and, per name of ``want``,
    a list of the groups' per-sample arrays.  ``device_ptrs``: {"theta": [addresses or None per group], "z": [...]} to
    have the draws written to the caller's device memory instead (no host ``theta`` / ``z`` is then returned).  ``skip``: per-group
    outputs to pass as NULL (tests)."""
    lib = _laplace_lib.load()
    G, S = len(xs), int(n_samples)
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    xs, fluxes, noises = [f64(x) for x in xs], [f64(f) for f in fluxes], [f64(n) for n in noises]
    bounds, centres, chols = [f64(b) for b in bounds], [f64(c) for c in centres], [f64(c) for c in chols]
    for x, f, n in zip(xs, fluxes, noises):
        if x.ndim != 1 or f.shape != x.shape or (n is not None and n.shape != x.shape):
            raise ValueError("flux and noise must have the abscissa's shape")
    dims = [Q_OF_MODE.get(m, 3) * k + sd for m, k, sd in zip(modes, n_comp, sample_sd)]
    n_vec, n_mat = int(sum(dims)), int(sum(d * d for d in dims))
    big = 0 < S <= MAX_SAMPLES and all(0 < d <= 4 * MAX_COMPONENTS + 1 for d in dims)     # (the library refuses the rest)
    out = {k: np.empty(G) for k in _GRP if k not in skip}
    out.update({k: np.empty(G, dtype=np.int32) for k in _CNT if k not in skip})
    out.update({k: np.empty(n_vec) for k in _VEC if k not in skip})
    if "cov" not in skip:
        out["cov"] = np.empty(n_mat)
    samples = {k: [np.empty((S, d)) if big else None for d in dims] for k in _SAMPLE_MAT if k in want and not device_ptrs}
    samples.update({k: [np.empty(S) if big else None for _ in dims] for k in _SAMPLE_VEC if k in want})
    ptrs = lambda arrays: (C.c_void_p * G)(*[None if a is None else a.ctypes.data for a in arrays])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_IP)
    arg = lambda k, ty: out[k].ctypes.data_as(ty) if k in out else None

    def sample_arg(k):
        if device_ptrs and k in _SAMPLE_MAT:
            return (C.c_void_p * G)(*[None if p is None else int(p) for p in device_ptrs[k]]) if k in device_ptrs else None
        return ptrs(samples[k]) if k in samples else None

    _laplace_lib.check(lib.vamp_laplace_points(
        int(device), C.c_void_p(stream or 0), G, ptrs(xs), ptrs(fluxes), ptrs(noises), i32([x.size for x in xs]), i32(n_comp), i32(modes),
        i32(sample_sd), ptrs(bounds), i32(region_ids), ptrs(centres), ptrs(chols), S, int(seed) & (2 ** 64 - 1),
        *[arg(k, _DP) for k in _GRP], *[arg(k, _IP) for k in _CNT], *[arg(k, _DP) for k in _VEC + ("cov",)],
        sample_arg("theta"), sample_arg("z"), int(bool(device_ptrs)), *[sample_arg(k) for k in _SAMPLE_VEC]), lib)
    out.update(samples)
    return out


def _split(flat, dims, n_samples, inflate, logdets, want):
    """the outputs of ``_call`` as one record per group; logdets: ln det of the information behind every proposal"""
    recs, ov, om = [], 0, 0
    for g, D in enumerate(dims):
        f = {k: float(flat[k][g]) for k in _GRP}
        f.update({k: int(flat[k][g]) for k in _CNT})
        f.update({k: flat[k][ov:ov + D].copy() for k in _VEC}, cov=flat["cov"][om:om + D * D].reshape(D, D).copy())
        f.update({k: flat[k][g] for k in _SAMPLES if k in want and k in flat})
        f.update(lnZ_laplace=f["lnp_centre"] + 0.5 * D * math.log(2.0 * math.pi) - 0.5 * float(logdets[g]), n_samples=int(n_samples),
                 inflate=float(inflate))
        recs.append(LaplaceRecord(**f))
        ov, om = ov + D, om + D * D
    return recs


def proposal_factor(cov, inflate=1.5, status=0):
    """(the lower Cholesky factor of inflate^2 cov, ln det of cov^-1): a covariance that does not factor, or one whose
    Fisher ``status`` is not 0, gives a NaN factor, which the library answers with status 1"""
    cov = np.asarray(cov, dtype=np.float64)
    D = cov.shape[0]
    if status == 0 and np.isfinite(cov).all():
        try:
            c = np.linalg.cholesky(float(inflate) ** 2 * cov)
            return np.ascontiguousarray(c), -2.0 * (float(np.sum(np.log(np.diag(c)))) - D * math.log(float(inflate)))
        except np.linalg.LinAlgError:
            pass
    return np.full((D, D), np.nan), float("nan")


def laplace_points(xs, fluxes, noises, centres, covs, n_comp, mode, n_samples=4096, inflate=1.5, seed=DEFAULT_SEED, bounds=None, device=0,
                   want=(), region_ids=None, statuses=None):
    """Records of one region -- ``xs`` a 1-D abscissa, ``centres`` [D], ``covs`` [D, D] (returns a record) -- or of a list
    of regions (returns a list), all in one library call.  The proposal of a region is N(centre, inflate^2 cov): ``covs``
    is the Fisher covariance at the centre (``fisher.fisher_points(...).cov``), ``statuses`` its status (a region whose
    status is not 0, or whose covariance does not factor, gets status 1).  A noise of ``None`` means free sd: the centre's
    last entry.  ``n_comp``, ``mode`` (0 = Gauss, 1 = Voigt) and ``bounds`` ((c_lo, c_hi, sigma_max, fwhm_max), or None to
    derive them from x as ``evidence.log_evidence`` does) are one value for all, or one per region; ``region_ids`` (default:
    the positions) key the draws.  ``want``: per-sample outputs to keep, of "theta", "z", "lnp", "lnq", "lw"."""
    single = isinstance(xs, np.ndarray) and xs.ndim == 1
    if single:
        xs, fluxes, noises, centres, covs = [xs], [fluxes], [noises], [centres], [covs]
        bounds = None if bounds is None else [bounds]
    xs, fluxes, noises, centres, covs = list(xs), list(fluxes), list(noises), list(centres), list(covs)
    if not len(xs) == len(fluxes) == len(noises) == len(centres) == len(covs):
        raise ValueError("one abscissa, one flux, one noise (or None), one centre and one covariance per region are required")
    G = len(xs)
    if G == 0:
        return []
    n_comp, modes = per_group(n_comp, G, int), per_group(mode, G, int)
    if bounds is not None and np.ndim(bounds[0] if len(bounds) else 0) == 0:
        bounds = [bounds] * G
    bounds = [None] * G if bounds is None else list(bounds)
    region_ids = list(range(G)) if region_ids is None else [int(r) for r in region_ids]
    statuses = [0] * G if statuses is None else [int(s) for s in statuses]
    if not len(bounds) == len(region_ids) == len(statuses) == G:
        raise ValueError("one bounds, one region id and one status per region are required")
    sds = [int(n is None) for n in noises]
    centres = [np.ascontiguousarray(c, dtype=np.float64) for c in centres]
    covs = [np.asarray(c, dtype=np.float64) for c in covs]
    for c, v, k, m, sd, b in zip(centres, covs, n_comp, modes, sds, bounds):
        if m not in Q_OF_MODE:
            raise ValueError(f"mode {m} is not supported (0 = Gauss, 1 = Voigt)")
        if not 1 <= k <= MAX_COMPONENTS:
            raise ValueError(f"n_comp = {k} is outside 1 .. {MAX_COMPONENTS}")
        D = Q_OF_MODE[m] * k + sd
        if c.shape != (D,):
            raise ValueError(f"a centre of shape {c.shape} does not hold {k} lines of mode {m} (free sd = {bool(sd)})")
        if v.shape != (D, D):
            raise ValueError(f"a covariance of shape {v.shape} does not belong to a centre of {D} parameters")
        if b is not None and np.shape(b) != (4,):
            raise ValueError("bounds must be (c_lo, c_hi, sigma_max, fwhm_max)")
    if not inflate > 0:
        raise ValueError("inflate must be positive")
    unknown = set(want) - set(_SAMPLES)
    if unknown:
        raise ValueError(f"unknown per-sample outputs {sorted(unknown)}")
    factors = [proposal_factor(v, inflate, st) for v, st in zip(covs, statuses)]
    dims = [c.size for c in centres]
    flat = _call(int(device), xs, fluxes, noises, n_comp, modes, sds, bounds, region_ids, centres, [f[0] for f in factors], n_samples, seed,
                 want=tuple(want))
    recs = _split(flat, dims, n_samples, inflate, [f[1] for f in factors], want)
    return recs[0] if single else recs


def fits_laplace(fits, n_samples=4096, inflate=1.5, seed=DEFAULT_SEED, device=0, want=(), metric="fisher"):
    """Records of many ``VPfit`` objects at their current point (``fit._theta_dev``: the MAP after ``map_estimate``): ONE
    ``fisher.fits_fisher`` call for the proposals' covariances, then ONE library call.  The bounds are those the library
    derives from the abscissa, as for ``evidence.log_evidence``; the draws are keyed by the fits' positions.  The records
    are in the caller's units (the affine map of ``VPfit._to_caller``) and named with the fits' parameter names; each fit's
    ``laplace()`` cache is filled.  Returns the records, one per fit.

    ``metric``: "fisher" is the above.  "regularised" and "chain" take the proposal's covariance from
    ``metric.fits_metric`` (source "fisher" / "chain") instead, so a region whose information is singular or indefinite
    still gets a proposal; ``status`` 1 then means a metric status other than 0, ``lnZ_laplace`` uses the regularised
    information, and the records carry ``n_low`` and ``n_high``."""
    fits = list(fits)
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r} is not one of {METRICS}")
    if not fits:
        return []
    repaired = None
    if metric == "fisher":
        from . import fisher
        fish = fisher.fits_fisher(fits, device=device)
        # the Fisher records are in the caller's units: back to the device units the centre is in
        covs = [r.cov / np.outer(f._scale, f._scale) for f, r in zip(fits, fish)]
    else:
        from . import metric as metric_mod
        fish = repaired = metric_mod.fits_metric(fits, source="fisher" if metric == "regularised" else "chain", device=device)
        covs = [np.asarray(r.cov, dtype=np.float64) for r in repaired]
    recs = laplace_points([f._x for f in fits], [f._flux for f in fits], [None if f._sample_sd else f.noise for f in fits],
                          [np.asarray(f._theta_dev, dtype=np.float64) for f in fits], covs, [f._n for f in fits], [int(f._mode) for f in fits],
                          n_samples=n_samples, inflate=inflate, seed=seed, device=device, want=want, statuses=[r.status for r in fish])
    out = []
    for i, (f, r) in enumerate(zip(fits, recs)):
        r.metric = metric
        if repaired is not None:
            r.n_low, r.n_high = int(repaired[i].n_low), int(repaired[i].n_high)
        rec = r.to_units(f._scale, f._shift, names=f._names)
        f._set_laplace(rec, (int(n_samples), float(inflate), int(seed)) + (() if metric == "fisher" else (metric,)))
        out.append(rec)
    return out
