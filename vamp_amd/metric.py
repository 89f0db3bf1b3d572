"""A positive-definite metric from any symmetric matrix, on the GPU (libvamp_metric.so, include/vamp_metric.h; definitions:
DESIGN.md section 18).  The matrix -- an information that may be singular or indefinite, or a covariance that may be
degenerate or wider than the prior -- is written in units of each parameter's prior standard deviation, decomposed by
Jacobi's method, its eigenvalues clamped to [lam_lo, lam_hi], and turned into a covariance, a precision, ln det and the
Cholesky factor ``hmc.hmc_points`` and ``laplace.laplace_points`` take.  ``n_low`` says how many directions the data
constrain less than the prior does: they get the prior's width.

    regularise(mats, scales, kind="info", ...)          the raw call: host matrices and scales
    prior_scales(x, n_comp, mode, sample_sd)            the prior standard deviations, in device units
    fits_metric(fits, source="fisher" | "chain", ...)   many VPfit objects at their current point

Each ``regularise`` call is ONE library call for all the matrices it is given.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _metric_lib
from ._sidelib import Q_OF_MODE, per_group

MAX_DIM, MAX_SWEEPS = 65, 32                  # of include/vamp_metric.h
# the restatement's largest sweep count over the test families at D = 65 (the empty sweep included), plus 4
# (tests/test_metric.py measures it; profiles/metric_limits.txt)
DEFAULT_SWEEPS = 20
KINDS = {"info": 0, "cov": 1}
SOURCES = ("fisher", "chain")

_MAT, _VEC, _PT, _CNT = ("vec", "cov", "prec", "chol"), ("eig",), ("logdet", "off"), ("n_low", "n_high", "sweeps_used", "status")
FIELDS = ("chol", "cov", "prec", "eig", "vec", "logdet", "n_low", "n_high", "sweeps_used", "off", "status")
OPTIONAL = ("vec", "prec")                    # returned when asked for (``want``)
_DP, _IP, _LP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class MetricRecord:
    """One matrix's ``chol`` [D, D] (the lower factor of ``cov``), ``cov`` and ``prec`` [D, D] (the regularised covariance
    and its inverse), ``eig`` [D] (the eigenvalues of the matrix in prior units, ascending) and ``vec`` [D, D] (their
    vectors, in columns), ``logdet`` (ln det of the regularised information), ``n_low`` / ``n_high`` (eigenvalues of the
    information below ``lam_lo`` / above ``lam_hi``), ``sweeps_used``, ``off`` (the largest off-diagonal entry left) and
    ``status`` (0 ok; 1 cov does not factor: no chol; 2 an entry is not finite: everything NaN; 3 not converged: eig and
    vec only).  A group of M matrices has every field with a leading axis of M.  ``vec`` and ``prec`` are None unless
    asked for."""

    __slots__ = FIELDS

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields.get(k))

    def __repr__(self):
        return f"MetricRecord(D={None if self.eig is None else np.shape(self.eig)[-1]}, status={self.status!r}, n_low={self.n_low!r}, n_high={self.n_high!r})"


def plan(max_dim):
    """(matrices per workgroup, bytes of dynamic LDS per workgroup) of a call whose largest D is ``max_dim``"""
    lib = _metric_lib.load()
    n, b = C.c_int32(0), C.c_int64(0)
    _metric_lib.check(lib.vamp_metric_plan(int(max_dim), C.byref(n), C.byref(b)), lib)
    return int(n.value), int(b.value)


def _call(device, mats, ld, dims, n_mats, scales, kinds, lam_lo, lam_hi, n_sweeps, is_device=False, stream=None, device_out=None, skip=()):
    """One vamp_metric_factor call; returns the flat outputs by name.  ``mats``: contiguous fp64 host arrays, or device
    addresses with ``is_device``.  ``device_out``: {"cov": address, "chol": address} to have those written to the caller's
    device memory (no host array of them is then returned).  ``skip``: outputs to pass as NULL (tests)."""
    lib = _metric_lib.load()
    G = len(mats)
    sane = all(1 <= int(d) <= MAX_DIM for d in dims) and all(0 < int(m) < (1 << 24) for m in n_mats)       # (the library refuses the rest)
    n_pt = sum(int(m) for m in n_mats) if sane else 0
    n_vec = sum(int(m) * int(d) for m, d in zip(n_mats, dims)) if sane else 0
    n_mat = sum(int(m) * int(d) ** 2 for m, d in zip(n_mats, dims)) if sane else 0
    out = {k: np.empty(n_mat) for k in _MAT if k not in skip and not (device_out and k in ("cov", "chol"))}
    out.update({k: np.empty(n_vec) for k in _VEC if k not in skip})
    out.update({k: np.empty(n_pt) for k in _PT if k not in skip})
    out.update({k: np.empty(n_pt, dtype=np.int32) for k in _CNT if k not in skip})
    scales = [np.ascontiguousarray(s, dtype=np.float64) for s in scales]
    addr = [int(m) if is_device else m.ctypes.data for m in mats]
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_IP)
    dbl = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_DP)
    arg = lambda k, ty: out[k].ctypes.data_as(ty) if k in out else None

    def mem(k):
        if device_out:
            return C.c_void_p(int(device_out[k])) if device_out.get(k) else None
        return C.c_void_p(out[k].ctypes.data) if k in out else None

    _metric_lib.check(lib.vamp_metric_factor(
        int(device), C.c_void_p(stream or 0), G, (C.c_void_p * G)(*addr), int(bool(is_device)),
        np.ascontiguousarray(ld, dtype=np.int64).ctypes.data_as(_LP), i32(dims), i32(n_mats), (C.c_void_p * G)(*[s.ctypes.data for s in scales]),
        i32(kinds), dbl(lam_lo), dbl(lam_hi), int(n_sweeps), int(bool(device_out)), arg("eig", _DP), arg("vec", _DP), mem("cov"), arg("prec", _DP),
        mem("chol"), arg("logdet", _DP), arg("n_low", _IP), arg("n_high", _IP), arg("sweeps_used", _IP), arg("off", _DP), arg("status", _IP)), lib)
    return out


def _split(flat, dims, n_mats, stacked, want):
    """the outputs of ``_call`` as one record per group"""
    recs, ov, om, op = [], 0, 0, 0
    for D, M, st in zip(dims, n_mats, stacked):
        f = {k: flat[k][om:om + M * D * D].reshape(M, D, D).copy() for k in _MAT if k in flat and (k not in OPTIONAL or k in want)}
        f.update({k: flat[k][ov:ov + M * D].reshape(M, D).copy() for k in _VEC})
        f.update({k: flat[k][op:op + M].copy() for k in _PT + _CNT})
        if not st:
            f = {k: (v[0] if v.ndim > 1 else (int(v[0]) if k in _CNT else float(v[0]))) for k, v in f.items()}
        recs.append(MetricRecord(**f))
        ov, om, op = ov + M * D, om + M * D * D, op + M
    return recs


def regularise(mats, scales, kind="info", lam_lo=1.0, lam_hi=2.0 ** 40, n_sweeps=None, device=0, want=()):
    """Records of one matrix -- ``mats`` [D, D], ``scales`` [D] (returns a record) -- or of a list of groups (returns a
    list), all in one library call; a group is one matrix [D, D] or M matrices [M, D, D] that share their scales.  Only
    the lower triangles are read.  ``scales``: the prior standard deviations of the parameters (``prior_scales``), in the
    matrix's units.  ``kind``: "info" (informations: inverse covariances) or "cov" (covariances); ``kind``, ``lam_lo`` and
    ``lam_hi`` are one value for all, or one per group.  In prior units an eigenvalue of the information below ``lam_lo``
    = 1 is a direction the data constrain less than the prior: it is raised to ``lam_lo``.  ``lam_hi`` = 2^40 is a default,
    not a measurement: it keeps the condition of ``cov`` in prior units below the 2e13 to which the Fisher tests carry the
    same Cholesky rule; ``math.inf`` switches it off.  ``n_sweeps`` (None: ``DEFAULT_SWEEPS``, measured on the test
    families at D = 65) bounds the Jacobi sweeps; a matrix that needs more gets status 3.  ``want``: of "vec", "prec"."""
    single = isinstance(mats, np.ndarray) and mats.ndim == 2 and np.ndim(scales) == 1
    if single or (isinstance(mats, np.ndarray) and mats.ndim == 3 and np.ndim(scales) == 1):
        mats, scales = [mats], [scales]
    mats, scales = list(mats), list(scales)
    if len(mats) != len(scales):
        raise ValueError("one set of scales per group of matrices is required")
    G = len(mats)
    if G == 0:
        return []
    kinds = per_group(kind, G, str)
    lam_lo, lam_hi = per_group(lam_lo, G, float), per_group(lam_hi, G, float)
    if not len(kinds) == len(lam_lo) == len(lam_hi) == G:
        raise ValueError("one kind, one lam_lo and one lam_hi per group are required")
    n_sweeps = DEFAULT_SWEEPS if n_sweeps is None else int(n_sweeps)
    if not 1 <= n_sweeps <= MAX_SWEEPS:
        raise ValueError(f"n_sweeps = {n_sweeps} is outside 1 .. {MAX_SWEEPS}")
    unknown = set(want) - set(OPTIONAL)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    mats = [np.ascontiguousarray(m, dtype=np.float64) for m in mats]
    scales = [np.ascontiguousarray(s, dtype=np.float64) for s in scales]
    for m, s, k, lo, hi in zip(mats, scales, kinds, lam_lo, lam_hi):
        if k not in KINDS:
            raise ValueError(f"kind {k!r} is not one of {sorted(KINDS)}")
        if m.ndim not in (2, 3) or m.shape[-1] != m.shape[-2] or m.shape[0] < 1:
            raise ValueError(f"a group of shape {m.shape} is neither [D, D] nor [M, D, D]")
        D = m.shape[-1]
        if not 1 <= D <= MAX_DIM:
            raise ValueError(f"D = {D} is outside 1 .. {MAX_DIM}")
        if s.shape != (D,):
            raise ValueError(f"scales of shape {s.shape} do not belong to matrices of {D} parameters")
        if not (np.isfinite(s).all() and np.all(s > 0)):
            raise ValueError("scales must be positive and finite")
        if not (lo > 0 and math.isfinite(lo) and hi >= lo):
            raise ValueError("0 < lam_lo <= lam_hi is required, lam_lo finite")
    dims = [m.shape[-1] for m in mats]
    stacked = [m.ndim == 3 for m in mats]
    n_mats = [m.shape[0] if st else 1 for m, st in zip(mats, stacked)]
    flat = _call(int(device), mats, dims, dims, n_mats, scales, [KINDS[k] for k in kinds], lam_lo, lam_hi, n_sweeps,
                 skip=tuple(k for k in OPTIONAL if k not in want))
    recs = _split(flat, dims, n_mats, stacked, tuple(want))
    return recs[0] if single else recs


def prior_scales(x, n_comp, mode, sample_sd):
    """the standard deviations of the library's priors [D], in the units of the abscissa ``x`` (a fit's device units):
    sqrt(2) for amplitudes (the prior A e^-A), (c_hi - c_lo) / sqrt(12) for centres and w_max / sqrt(12) for widths (uniform on
    the ranges ``hmc.derived_bounds`` gives), 1 / sqrt(12) for the free sd (uniform on (0, 1))"""
    from .hmc import derived_bounds
    if mode not in Q_OF_MODE:
        raise ValueError(f"mode {mode} is not supported (0 = Gauss, 1 = Voigt)")
    lo, hi, wmax = derived_bounds(x, mode)
    r12 = math.sqrt(12.0)
    line = [math.sqrt(2.0), (hi - lo) / r12] + [wmax / r12] * (Q_OF_MODE[mode] - 2)
    return np.array(line * int(n_comp) + ([1.0 / r12] if sample_sd else []), dtype=np.float64)


def chain_covariance(chain):
    """the sample covariance [D, D] of a chain [N, W, D], all walkers pooled (numpy, on the host)"""
    s = np.asarray(chain, dtype=np.float64)
    s = s.reshape(-1, s.shape[-1])
    return np.atleast_2d(np.cov(s, rowvar=False))


def fits_metric(fits, source="fisher", lam_lo=1.0, lam_hi=2.0 ** 40, n_sweeps=None, device=0, want=()):
    """Records of many ``VPfit`` objects, in device units (those of ``fit._theta_dev`` on ``fit._x``), from ONE library call.
    ``source`` = "fisher": the information of ONE ``fisher.fits_fisher`` call at the fits' current points, taken back to
    device units by outer(scale, scale); a bad point (Fisher status 2) has a NaN information and gets status 2.
    ``source`` = "chain": the covariance of each fit's kept stretch-move chain (``fit._chain_dev``, numpy on the host); a
    fit without a chain raises."""
    fits = list(fits)
    if source not in SOURCES:
        raise ValueError(f"source {source!r} is not one of {SOURCES}")
    if not fits:
        return []
    if source == "fisher":
        from . import fisher
        fish = fisher.fits_fisher(fits, device=device)
        mats = [np.asarray(r.info, dtype=np.float64) * np.outer(f._scale, f._scale) for f, r in zip(fits, fish)]
        kind = "info"
    else:
        for f in fits:
            if getattr(f, "_chain_dev", None) is None:
                raise ValueError("source='chain' needs fits that have been sampled and still hold their chain")
        mats = [chain_covariance(f._chain_dev) for f in fits]
        kind = "cov"
    scales = [prior_scales(f._x, f._n, int(f._mode), bool(f._sample_sd)) for f in fits]
    return regularise(mats, scales, kind=kind, lam_lo=lam_lo, lam_hi=lam_hi, n_sweeps=n_sweeps, device=device, want=want)
