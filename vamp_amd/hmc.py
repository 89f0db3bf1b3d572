"""Preconditioned Hamiltonian Monte Carlo on the GPU: independent chains per region, each move L leapfrog steps in the
metric of a given factor, with the exact log-posterior and its analytic gradient (libvamp_hmc.so, include/vamp_hmc.h;
definitions: DESIGN.md section 17).  The kernel never adapts: the step size of a call is fixed per region.

    hmc_points(xs, fluxes, noises, starts, chols, n_comp, mode, eps, ...)      the raw call: host starts and factors
    fits_hmc(fits, ...)                                                        many VPfit objects from their current point

Each ``hmc_points`` call is ONE library call for all the regions it is given.  Starts, factors and abscissae are in the
same units (a fit's device units: ``fit._theta_dev`` on ``fit._x``); ``fits_hmc`` hands back records in the caller's
units.  A ``noise`` of ``None`` means the vector's last entry is the free sd, the noise of every pixel.  A record's
``chain`` is [n_keep, C, D], the layout of every chain consumer (``diagnostics``, ``posterior``, ``predictive``, ``loo``,
``relabel``).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _hmc_lib
from ._sidelib import Q_OF_MODE, per_group

MAX_COMPONENTS, MAX_LEAP, MAX_CHAIN_ID = 16, 64, 1 << 26      # of include/vamp_hmc.h
DEFAULT_SEED = 20110101
QUANTILES = (0.16, 0.5, 0.84)
METRICS = ("fisher", "regularised", "chain")

_PER_CHAIN_I, _PER_CHAIN_D = ("n_accept", "n_wall", "chain_status"), ("dH_mean", "dH_max")
_TRACE_MAT, _TRACE_VEC = ("mom", "prop", "prop_mom"), ("dH",)
TRACES = _TRACE_MAT + _TRACE_VEC + ("acc",)
_DP, _IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def n_keep_of(n_steps, n_burn, thin):
    """the number of steps t >= n_burn with (t - n_burn) mod thin = 0"""
    return -(-(int(n_steps) - int(n_burn)) // int(thin))


class HmcRecord:
    """One region's ``chain`` [n_keep, C, D] and ``lnp`` [n_keep, C], per chain ``accept_rate`` (accepted steps / n_steps),
    ``n_wall`` (steps that left the prior), ``dH_mean`` / ``dH_max`` (of |dH| over the steps that met no wall) and
    ``chain_status`` (0 ok; 2 the start was rejected: that chain is NaN), ``status`` (0 ok; 1 no factor or no Fisher
    covariance: no chain), ``eps`` (the step size of the kept run), ``last`` [C, D] (the final state), ``n_steps``,
    ``n_leap``, ``thin``, ``names`` (the fit's parameter names when the record was made from a fit, else None), ``metric``
    (what ``fits_hmc`` took the factor from, else None) with ``n_low`` / ``n_high`` (the directions a regularised metric
    repaired; None with the Fisher metric) and -- when asked for, else None -- the per-step traces ``mom`` / ``prop`` / ``prop_mom`` [n_steps, C, D], ``dH`` and ``acc``
    [n_steps, C]."""

    __slots__ = ("chain", "lnp", "accept_rate", "n_wall", "dH_mean", "dH_max", "chain_status", "status", "eps", "last", "n_steps",
                 "n_leap", "thin", "names", "_diag", "metric", "n_low", "n_high") + TRACES

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields.get(k))

    def diagnostics(self, c=5.0, device=0):
        """tau, n_eff and split-R-hat per parameter of the chain (``vamp_amd.diagnostics.chain_diagnostics``; tau in kept
        samples of ``thin`` moves each).  Cached.  None when the record has no chain."""
        if self.chain is None:
            return None
        if self._diag is None or self._diag[0] != float(c):
            from . import diagnostics
            self._diag = (float(c), diagnostics.chain_diagnostics(self.chain, thin=self.thin or 1, c=c, device=device))
        return self._diag[1]

    def samples(self):
        """the chains of status 0 side by side: [n_keep * C_ok, D]"""
        ok = np.asarray(self.chain_status) == 0
        return self.chain[:, ok, :].reshape(-1, self.chain.shape[2])

    def summary(self):
        """(mean [D], sd [D], quantiles 0.16 / 0.5 / 0.84 [3, D]) over the chains of status 0; NaN without a chain"""
        if self.chain is None or not np.any(np.asarray(self.chain_status) == 0):
            D = 0 if self.last is None else self.last.shape[1]
            return np.full(D, np.nan), np.full(D, np.nan), np.full((3, D), np.nan)
        s = self.samples()
        return s.mean(axis=0), s.std(axis=0, ddof=1) if len(s) > 1 else np.full(s.shape[1], np.nan), np.quantile(s, QUANTILES, axis=0)

    def to_units(self, scale, shift=None, names=None):
        """the record of the same chains in units theta' = theta * scale + shift: chain, last and prop are mapped, the
        momenta (which live in the factor's metric) and everything else stay"""
        D = (self.last if self.last is not None else self.chain).shape[-1]
        s = np.asarray(scale, dtype=np.float64)
        if s.shape != (D,):
            raise ValueError(f"{s.size} scales for a record of {D} parameters")
        t = np.zeros_like(s) if shift is None else np.asarray(shift, dtype=np.float64)
        f = {k: getattr(self, k) for k in self.__slots__}
        move = lambda a: None if a is None else a * s + t
        f.update(chain=move(self.chain), last=move(self.last), prop=move(self.prop), names=self.names if names is None else list(names),
                 _diag=self._diag)          # (tau and R-hat are invariant under an affine map)
        return HmcRecord(**f)

    def __repr__(self):
        shape = None if self.chain is None else self.chain.shape
        acc = None if self.accept_rate is None else float(np.nanmean(self.accept_rate))
        return f"HmcRecord(chain={shape}, status={self.status}, eps={self.eps!r}, accept_rate={acc!r})"


def _call(device, xs, fluxes, noises, n_comp, modes, sample_sd, bounds, region_ids, n_chains, chain_id0, starts, chols, eps, jitter,
          n_leap, n_steps, n_burn=0, thin=1, step0=0, seed=DEFAULT_SEED, want=TRACES, mom_in=None, stream=None, device_ptrs=None, skip=()):
    """One vamp_hmc_chains call; returns per name a list over the groups (``chain``, ``last``, ``lnp`` and the traces in
    ``want``), the flat per-chain arrays and ``status`` [G].  ``device_ptrs``: {"start": [addresses], "chain": [addresses or
    None], "last": [...]} to read the starts from, and write the chains to, the caller's device memory (no host ``chain`` /
    ``last`` is then returned).  ``skip``: outputs to pass as NULL (tests)."""
    lib = _hmc_lib.load()
    G = len(xs)
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    xs, fluxes, noises = [f64(x) for x in xs], [f64(f) for f in fluxes], [f64(n) for n in noises]
    bounds, chols = [f64(b) for b in bounds], [f64(c) for c in chols]
    device_ptrs = device_ptrs or {}
    starts = [f64(s) for s in starts] if "start" not in device_ptrs else None
    mom_in = None if mom_in is None else [f64(m) for m in mom_in]
    for x, f, n in zip(xs, fluxes, noises):
        if x.ndim != 1 or f.shape != x.shape or (n is not None and n.shape != x.shape):
            raise ValueError("flux and noise must have the abscissa's shape")
    dims = [Q_OF_MODE.get(m, 3) * k + sd for m, k, sd in zip(modes, n_comp, sample_sd)]
    n_chains = [int(c) for c in n_chains]
    sane = 0 < int(n_steps) < (1 << 24) and 0 <= int(n_burn) < int(n_steps) and int(thin) >= 1 and all(0 < d <= 65 for d in dims) \
        and all(0 < c <= MAX_CHAIN_ID for c in n_chains)                       # (the library refuses the rest)
    keep = n_keep_of(n_steps, n_burn, thin) if sane else 0
    tot = sum(n_chains) if sane else 0
    out = {k: np.empty(tot, dtype=np.int32) for k in _PER_CHAIN_I if k not in skip}
    out.update({k: np.empty(tot) for k in _PER_CHAIN_D if k not in skip})
    if "status" not in skip:
        out["status"] = np.empty(G, dtype=np.int32)
    lists = {}
    out_dev = "chain" in device_ptrs or "last" in device_ptrs
    if sane:
        if not out_dev:
            lists.update({k: [np.empty((n, c, d)) for c, d in zip(n_chains, dims)] for k, n in (("chain", keep), ("last", 1)) if k not in skip})
        if "lnp" not in skip:
            lists["lnp"] = [np.empty((keep, c)) for c in n_chains]
        lists.update({k: [np.empty((int(n_steps), c, d)) for c, d in zip(n_chains, dims)] for k in _TRACE_MAT if k in want})
        lists.update({k: [np.empty((int(n_steps), c)) for c in n_chains] for k in _TRACE_VEC if k in want})
        if "acc" in want:
            lists["acc"] = [np.empty((int(n_steps), c), dtype=np.int32) for c in n_chains]
    ptrs = lambda arrays: None if arrays is None else (C.c_void_p * G)(*[None if a is None else a.ctypes.data for a in arrays])
    addr = lambda k: (C.c_void_p * G)(*[None if p is None else int(p) for p in device_ptrs[k]])
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_IP)
    dbl = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_DP)
    arg = lambda k, ty: out[k].ctypes.data_as(ty) if k in out else None
    lst = lambda k: ptrs(lists[k]) if k in lists else None
    state = lambda k: addr(k) if k in device_ptrs else (None if out_dev else lst(k))
    _hmc_lib.check(lib.vamp_hmc_chains(
        int(device), C.c_void_p(stream or 0), G, ptrs(xs), ptrs(fluxes), ptrs(noises), i32([x.size for x in xs]), i32(n_comp), i32(modes),
        i32(sample_sd), ptrs(bounds), i32(region_ids), i32(n_chains), i32(chain_id0), addr("start") if starts is None else ptrs(starts),
        int(starts is None), ptrs(chols), dbl(eps), dbl(jitter), int(n_leap), int(n_steps), int(n_burn), int(thin), int(step0),
        int(seed) & (2 ** 64 - 1), ptrs(mom_in), state("chain"), state("last"), int(out_dev), lst("lnp"), arg("n_accept", _IP),
        arg("n_wall", _IP), arg("dH_mean", _DP), arg("dH_max", _DP), arg("chain_status", _IP), arg("status", _IP), lst("mom"), lst("prop"),
        lst("prop_mom"), lst("dH"), lst("acc")), lib)
    if "last" in lists:
        lists["last"] = [a[0] for a in lists["last"]]
    out.update(lists)
    return out


def _split(flat, n_chains, eps, n_steps, n_leap, thin, want):
    """the outputs of ``_call`` as one record per group"""
    recs, o = [], 0
    for g, c in enumerate(n_chains):
        f = {k: flat[k][o:o + c].copy() for k in _PER_CHAIN_I + _PER_CHAIN_D}
        f.update({k: flat[k][g] for k in ("chain", "last", "lnp") + tuple(want) if k in flat})
        f.update(accept_rate=f.pop("n_accept") / float(n_steps), status=int(flat["status"][g]), eps=float(eps[g]), n_steps=int(n_steps),
                 n_leap=int(n_leap), thin=int(thin))
        if f["status"] != 0:
            f.update(chain=None, lnp=None)
        recs.append(HmcRecord(**f))
        o += c
    return recs


def _as_lists(xs, fluxes, noises, starts, chols, bounds):
    single = isinstance(xs, np.ndarray) and xs.ndim == 1
    if single:
        xs, fluxes, noises, starts, chols = [xs], [fluxes], [noises], [starts], [chols]
        bounds = None if bounds is None else [bounds]
    return single, list(xs), list(fluxes), list(noises), list(starts), list(chols), bounds


def hmc_points(xs, fluxes, noises, starts, chols, n_comp, mode, eps, n_steps=400, n_burn=0, thin=1, n_leap=8, jitter=0.2, seed=DEFAULT_SEED,
               bounds=None, device=0, want=(), region_ids=None, chain_id0=0, step0=0):
    """Records of one region -- ``xs`` a 1-D abscissa, ``starts`` [C, D], ``chols`` [D, D] (returns a record) -- or of a
    list of regions (returns a list), all in one library call.  ``chols``: the lower factor of the inverse mass matrix
    (the Cholesky factor of an estimate of the posterior covariance); ``eps``, ``jitter``, ``n_comp``, ``mode`` (0 = Gauss,
    1 = Voigt), ``chain_id0`` and ``bounds`` ((c_lo, c_hi, sigma_max, fwhm_max), or None to derive them from x as
    ``evidence.log_evidence`` does) are one value for all, or one per region; ``region_ids`` (default: the positions) key
    the draws.  A noise of ``None`` means free sd.  ``step0``: the steps already made, to continue a run from a record's
    ``last``.  ``want``: traces to keep, of "mom", "prop", "prop_mom", "dH", "acc"."""
    single, xs, fluxes, noises, starts, chols, bounds = _as_lists(xs, fluxes, noises, starts, chols, bounds)
    if not len(xs) == len(fluxes) == len(noises) == len(starts) == len(chols):
        raise ValueError("one abscissa, one flux, one noise (or None), one set of starts and one factor per region are required")
    G = len(xs)
    if G == 0:
        return []
    n_comp, modes = per_group(n_comp, G, int), per_group(mode, G, int)
    eps, jitter, chain_id0 = per_group(eps, G, float), per_group(jitter, G, float), per_group(chain_id0, G, int)
    if bounds is not None and np.ndim(bounds[0] if len(bounds) else 0) == 0:
        bounds = [bounds] * G
    bounds = [None] * G if bounds is None else list(bounds)
    region_ids = list(range(G)) if region_ids is None else [int(r) for r in region_ids]
    if not len(bounds) == len(region_ids) == len(eps) == len(jitter) == len(chain_id0) == G:
        raise ValueError("one bounds, one region id, one eps, one jitter and one chain_id0 per region are required")
    sds = [int(n is None) for n in noises]
    starts = [np.ascontiguousarray(s, dtype=np.float64) for s in starts]
    chols = [np.asarray(c, dtype=np.float64) for c in chols]
    for s, v, k, m, sd, b in zip(starts, chols, n_comp, modes, sds, bounds):
        if m not in Q_OF_MODE:
            raise ValueError(f"mode {m} is not supported (0 = Gauss, 1 = Voigt)")
        if not 1 <= k <= MAX_COMPONENTS:
            raise ValueError(f"n_comp = {k} is outside 1 .. {MAX_COMPONENTS}")
        D = Q_OF_MODE[m] * k + sd
        if s.ndim != 2 or s.shape[0] < 1 or s.shape[1] != D:
            raise ValueError(f"starts of shape {s.shape} do not hold chains of {k} lines of mode {m} (free sd = {bool(sd)})")
        if v.shape != (D, D):
            raise ValueError(f"a factor of shape {v.shape} does not belong to vectors of {D} parameters")
        if b is not None and np.shape(b) != (4,):
            raise ValueError("bounds must be (c_lo, c_hi, sigma_max, fwhm_max)")
    if not 1 <= int(n_leap) <= MAX_LEAP:
        raise ValueError(f"n_leap = {n_leap} is outside 1 .. {MAX_LEAP}")
    if not (int(n_steps) >= 1 and 0 <= int(n_burn) < int(n_steps) and int(thin) >= 1):
        raise ValueError("n_steps >= 1, 0 <= n_burn < n_steps and thin >= 1 are required")
    unknown = set(want) - set(TRACES)
    if unknown:
        raise ValueError(f"unknown traces {sorted(unknown)}")
    n_chains = [s.shape[0] for s in starts]
    flat = _call(int(device), xs, fluxes, noises, n_comp, modes, sds, bounds, region_ids, n_chains, chain_id0, starts, chols, eps, jitter,
                 n_leap, n_steps, n_burn, thin, step0, seed, want=tuple(want))
    recs = _split(flat, n_chains, eps, n_steps, n_leap, thin, tuple(want))
    return recs[0] if single else recs


def derived_bounds(x, mode):
    """(c_lo, c_hi, width_max) as the library derives them from the abscissa"""
    lo, hi = float(min(x[0], x[-1])), float(max(x[0], x[-1]))
    smax = (hi - lo) / 2.0
    return lo, hi, smax if mode == 0 else smax * 2.0 * math.sqrt(2.0 * math.log(2.0))


def inside_prior(theta, n_comp, mode, sample_sd, c_lo, c_hi, w_max):
    """whether the rows of theta [n, D] lie inside the library's prior (amplitudes > 0, centres and widths in their ranges,
    widths > 0 but for L_fwhm >= 0, 0 < sd <= 1)"""
    theta = np.atleast_2d(theta)
    q = Q_OF_MODE[mode]
    lines = theta[:, :q * n_comp].reshape(len(theta), n_comp, q)
    with np.errstate(invalid="ignore"):
        ok = np.all((lines[:, :, 0] > 0) & np.isfinite(lines[:, :, 0]) & (lines[:, :, 1] >= c_lo) & (lines[:, :, 1] <= c_hi), axis=1)
        if mode == 1:
            ok &= np.all((lines[:, :, 2] >= 0) & (lines[:, :, 2] <= w_max) & (lines[:, :, 3] > 0) & (lines[:, :, 3] <= w_max), axis=1)
        else:
            ok &= np.all((lines[:, :, 2] > 0) & (lines[:, :, 2] <= w_max), axis=1)
        if sample_sd:
            ok &= (theta[:, -1] > 0) & (theta[:, -1] <= 1.0)
    return ok


def draw_starts(centre, chol, n_chains, rng, inside, tries=64):
    """[C, D] starts centre + C z, z from ``rng``; a start that ``inside`` rejects is redrawn, up to ``tries`` times, and then
    put on the centre"""
    centre = np.asarray(centre, dtype=np.float64)
    out = centre + rng.standard_normal((n_chains, centre.size)) @ np.tril(chol).T
    for _ in range(tries):
        bad = ~inside(out)
        if not bad.any():
            break
        out[bad] = centre + rng.standard_normal((int(bad.sum()), centre.size)) @ np.tril(chol).T
    out[~inside(out)] = centre
    return out


def tuned_eps(eps, accept, target_accept, factor=1.5):
    """one multiplicative step of every region's step size towards ``target_accept``: up by ``factor`` where the mean
    acceptance of the round was above the target, down by it where it was below (or not a number)"""
    eps, accept = np.asarray(eps, dtype=np.float64), np.asarray(accept, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(accept > target_accept, eps * factor, eps / factor)


def fits_hmc(fits, n_chains=16, n_steps=400, n_burn=100, thin=1, n_leap=8, target_accept=0.8, tune_rounds=6, tune_steps=40, jitter=0.2,
             seed=DEFAULT_SEED, device=0, want=(), metric="fisher"):
    """Records of many ``VPfit`` objects from their current point (``fit._theta_dev``: the MAP after ``map_estimate``).  ONE
    ``fisher.fits_fisher`` call gives every region's covariance, whose Cholesky factor C is the metric; a region whose
    Fisher status is not 0 (or whose covariance does not factor) gets ``status`` 1 and no chain.  The chains start at MAP +
    C z with z from ``numpy.random.default_rng(seed)`` (a start outside the prior is redrawn).  The step size is tuned per
    region by ``tune_rounds`` short calls of ``tune_steps`` moves, each at a fixed eps per region and each starting where the
    one before ended: eps moves by a factor 1.5, then 1.25 from the third round on, towards ``target_accept``; the tuning
    chains are discarded and the kept run of ``n_steps`` moves (the first ``n_burn`` dropped) starts from their end.  The
    bounds are those the library derives from the abscissa; the draws are keyed by the fits' positions.  Records are in
    the caller's units and named with the fits' parameter names.

    The defaults -- n_steps = 400 with n_burn = 100, six tuning rounds of 40 moves, the starting eps = D^(-1/4) (the
    scaling of the optimal step of a D-dimensional standard normal) and the jitter 0.2 -- are choices that have not been
    measured until tools/bench_hmc.py has run (profiles/hmc_bench.txt).

    ``metric``: "fisher" is the above.  "regularised" takes the factor from ``metric.fits_metric(source="fisher")`` instead --
    the information in prior units with its eigenvalues below 1 raised to 1, so a region whose information is singular or
    indefinite still gets a metric -- and "chain" from ``metric.fits_metric(source="chain")``, the covariance of the fit's
    stretch-move chain treated alike.  ``status`` 1 then means a metric status other than 0, and the records carry
    ``n_low`` and ``n_high``."""
    fits = list(fits)
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r} is not one of {METRICS}")
    if not fits:
        return []
    if metric == "fisher":
        from . import fisher
        fish, repaired = fisher.fits_fisher(fits, device=device), None
    else:
        from . import metric as metric_mod
        repaired = metric_mod.fits_metric(fits, source="fisher" if metric == "regularised" else "chain", device=device)
        fish = repaired
    rng = np.random.default_rng(int(seed))
    G = len(fits)
    chols, starts, usable = [], [], []
    for f, r in zip(fits, fish):
        D = len(f._scale)
        chol = np.full((D, D), np.nan)
        if repaired is not None:
            if r.status == 0:
                chol = np.asarray(r.chol, dtype=np.float64)
        else:
            cov = r.cov / np.outer(f._scale, f._scale)             # back to the device units the point is in
            if r.status == 0 and np.isfinite(cov).all():
                try:
                    chol = np.linalg.cholesky(cov)
                except np.linalg.LinAlgError:
                    pass
        ok = bool(np.isfinite(chol).all())
        mode = int(f._mode)
        centre = np.asarray(f._theta_dev, dtype=np.float64)
        lo, hi, wmax = derived_bounds(f._x, mode)
        inside = lambda t, f=f, mode=mode, lo=lo, hi=hi, wmax=wmax: inside_prior(t, f._n, mode, bool(f._sample_sd), lo, hi, wmax)
        starts.append(draw_starts(centre, chol, int(n_chains), rng, inside) if ok else np.tile(centre, (int(n_chains), 1)))
        chols.append(chol)
        usable.append(ok)
    data = ([f._x for f in fits], [f._flux for f in fits], [None if f._sample_sd else f.noise for f in fits])
    ks, modes = [f._n for f in fits], [int(f._mode) for f in fits]
    eps = np.array([len(f._scale) ** -0.25 for f in fits])
    state, step0 = starts, 0
    for rnd in range(int(tune_rounds)):
        recs = hmc_points(*data, state, chols, ks, modes, eps, n_steps=tune_steps, n_burn=tune_steps - 1, n_leap=n_leap, jitter=jitter,
                          seed=seed, device=device, step0=step0)
        acc = np.array([np.nanmean(r.accept_rate) if r.status == 0 else np.nan for r in recs])
        eps = tuned_eps(eps, acc, target_accept, 1.5 if rnd < 2 else 1.25)
        # a chain whose start was rejected stays where it was
        state = [np.where(np.isfinite(r.last), r.last, s) if r.last is not None else s for r, s in zip(recs, state)]
        step0 += int(tune_steps)
    recs = hmc_points(*data, state, chols, ks, modes, eps, n_steps=n_steps, n_burn=n_burn, thin=thin, n_leap=n_leap, jitter=jitter, seed=seed,
                      device=device, want=want, step0=step0)
    out = []
    for i, (f, r) in enumerate(zip(fits, recs)):
        r.metric = metric
        if repaired is not None:
            r.n_low, r.n_high = int(repaired[i].n_low), int(repaired[i].n_high)
        out.append(r.to_units(f._scale, f._shift, names=f._names))
    return out
