"""Log-evidence ln Z of absorption regions from a ladder of tempered ensembles on the GPU (libvamp_evid.so,
include/vamp_evid.h; definitions: DESIGN.md "Evidence").

    log_evidence(regions, ...)       regions given as dicts of host arrays
    fits_evidence(fits, ...)         the regions of many VPfit objects
    lnlike(region, theta)            the device's ln L / ln pi of parameter vectors (test hook)

Each call is ONE library call for all the regions it is given.  A region is a dict with ``x``, ``flux``, ``noise``
(None with ``sample_sd``), ``n_comp``, ``mode`` (0 = Gauss: (A, c, sigma) per line, 1 = Voigt: (A, c, L_fwhm, G_fwhm)),
and optionally ``sample_sd``, ``bounds`` (c_lo, c_hi, sigma_max, fwhm_max) and ``region_id`` (default: its position).
Limits: n_comp <= 8, walkers <= 256 (even), 2 <= n_temps <= 64, fp64, no NBZ3.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _evid_lib
from ._sidelib import Q_OF_MODE

MAX_COMPONENTS, MAX_WALKERS, MAX_TEMPS = 8, 256, 64      # of include/vamp_evid.h
DEFAULT_SEED = 20110101
_DP, _IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class Evidence:
    """ln Z of one region: ``lnZ`` (stepping stone), ``lnZ_se`` (from 8 time blocks), ``lnZ_ti`` (trapezoid of the mean
    ln L over beta, a diagnostic), ``betas`` [T], ``mean_lnL`` / ``var_lnL`` / ``move_accept`` [T], ``swap_accept``
    [T - 1], and -- when asked for -- the beta = 1 rung's kept ``chain`` [n_keep, W, D] with its ``chain_lnl``
    [n_keep, W] (else None).  ``lnl_trace`` / ``swap_trace``: see the header (tests).  ``n_comp`` / ``mode`` /
    ``sample_sd``: the layout of ``chain``, which ``relabel()`` reads."""

    __slots__ = ("lnZ", "lnZ_se", "lnZ_ti", "betas", "mean_lnL", "var_lnL", "move_accept", "swap_accept", "chain", "chain_lnl",
                 "lnl_trace", "swap_trace", "n_comp", "mode", "sample_sd", "_relabel")

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields.get(k))

    def relabel(self, max_iter=10, device=0):
        """The ``RelabelRecord`` (vamp_amd.relabel) of the kept beta = 1 chain, with the relabelled chain in its
        ``chain``.  The ensemble started from independent prior draws, so every walker carries its own labelling and
        ``chain`` cannot be summarised per line as it stands.  The reference is the sample of highest ln L.  Cached per
        ``max_iter``."""
        if self.chain is None or self.chain_lnl is None or self.n_comp is None:
            raise RuntimeError("no chain: ask for it with return_chain=True")
        cache = self._relabel if self._relabel is not None else {}
        self._relabel = cache
        if int(max_iter) not in cache:
            from . import relabel
            K, q = int(self.n_comp), Q_OF_MODE[int(self.mode)]
            with np.errstate(invalid="ignore"):
                t, w = np.unravel_index(np.nanargmax(self.chain_lnl), self.chain_lnl.shape)
            ref = self.chain[t, w, :K * q].reshape(K, q)
            cache[int(max_iter)] = relabel.relabel_chains(self.chain, K, int(self.mode), int(bool(self.sample_sd)), ref, max_iter=max_iter,
                                                          device=device, return_chain=True)
        return cache[int(max_iter)]

    def __repr__(self):
        return f"Evidence(lnZ={self.lnZ!r}, lnZ_se={self.lnZ_se!r}, lnZ_ti={self.lnZ_ti!r}, T={len(self.betas)})"


def default_betas(n_temps):
    """beta_j = (j / (T - 1))^(1 / 0.3), the stepping-stone ladder of Xie et al. (2011)"""
    out = np.empty(int(n_temps))
    _evid_lib.check(_evid_lib.load().vamp_evid_default_betas(int(n_temps), out.ctypes.data_as(_DP)))
    return out


def _spec(region, position):
    """a region dict with contiguous fp64 arrays and every optional key filled"""
    sd = bool(region.get("sample_sd", False))
    sp = {"x": np.ascontiguousarray(region["x"], dtype=np.float64), "flux": np.ascontiguousarray(region["flux"], dtype=np.float64),
          "noise": None if region.get("noise") is None else np.ascontiguousarray(region["noise"], dtype=np.float64),
          "n_comp": int(region["n_comp"]), "mode": int(region.get("mode", 0)), "sample_sd": sd,
          "bounds": None if region.get("bounds") is None else np.ascontiguousarray(region["bounds"], dtype=np.float64),
          "region_id": int(region.get("region_id", position))}
    if sp["x"].ndim != 1 or sp["flux"].shape != sp["x"].shape or (sp["noise"] is not None and sp["noise"].shape != sp["x"].shape):
        raise ValueError("x, flux and noise must be one-dimensional arrays of one length")
    if sp["noise"] is None and not sd:
        raise ValueError("a region without noise needs sample_sd")
    if sp["bounds"] is not None and sp["bounds"].shape != (4,):
        raise ValueError("bounds must be (c_lo, c_hi, sigma_max, fwhm_max)")
    return sp


def _ptr(a):
    return None if a is None else a.ctypes.data


def lnlike(region, theta, device=0):
    """(ln L, ln pi) of the rows of ``theta`` [n, D] by the device function the sampler uses"""
    sp = _spec(region, 0)
    theta = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
    D = Q_OF_MODE.get(sp["mode"], 3) * sp["n_comp"] + int(sp["sample_sd"])
    if theta.shape[1] != D:
        raise ValueError(f"theta has {theta.shape[1]} parameters per row, the region {D}")
    ll, lp = np.empty(theta.shape[0]), np.empty(theta.shape[0])
    dp = lambda a: None if a is None else a.ctypes.data_as(_DP)
    lib = _evid_lib.load()
    _evid_lib.check(lib.vamp_evid_lnlike(int(device), dp(sp["x"]), dp(sp["flux"]), dp(sp["noise"]), sp["x"].size, sp["n_comp"], sp["mode"],
                                         int(sp["sample_sd"]), dp(sp["bounds"]), theta.shape[0], dp(theta), dp(ll), dp(lp)), lib)
    return ll, lp


def _run(specs, betas, walkers, steps, burn, swap_every, seed, a, starts, device, want_chain, want_trace=False):
    """One vamp_evid_run call; returns one dict per region (tests put the numpy restatement here)."""
    lib = _evid_lib.load()
    G, T, W = len(specs), len(betas), int(walkers)
    n_keep, n_swaps = int(steps) - int(burn), (int(steps) - 1) // max(1, int(swap_every))
    vp = lambda seq: (C.c_void_p * G)(*[_ptr(a) for a in seq])
    i32 = lambda seq: np.ascontiguousarray(seq, dtype=np.int32)
    n_pix, n_comp, modes, sds, ids = (i32(v) for v in ([s["x"].size for s in specs], [s["n_comp"] for s in specs], [s["mode"] for s in specs],
                                                       [int(s["sample_sd"]) for s in specs], [s["region_id"] for s in specs]))
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    starts = [None if s is None else np.ascontiguousarray(s, dtype=np.float64) for s in (starts or [None] * G)]
    out = {k: np.empty(n) for k, n in (("lnZ", G), ("lnZ_se", G), ("lnZ_ti", G), ("mean_lnL", G * T), ("var_lnL", G * T),
                                       ("move_accept", G * T), ("swap_accept", G * (T - 1)))}
    ok = n_keep > 0 and 0 < W <= MAX_WALKERS and 0 < T <= MAX_TEMPS        # (the library refuses the rest; no big allocation for it)
    dims = [Q_OF_MODE.get(s["mode"], 3) * s["n_comp"] + int(s["sample_sd"]) for s in specs]
    chains = [np.empty((n_keep, W, D)) if want_chain and ok else None for D in dims]
    chain_ll = [np.empty((n_keep, W)) if want_chain and ok else None for _ in specs]
    trace = np.empty((G, n_keep, T, W)) if want_trace and ok else None
    swaps = np.zeros((G, n_swaps, T - 1, W), dtype=np.uint8) if want_trace and ok else None
    _evid_lib.check(lib.vamp_evid_run(
        int(device), None, G, vp([s["x"] for s in specs]), vp([s["flux"] for s in specs]), vp([s["noise"] for s in specs]),
        n_pix.ctypes.data_as(_IP), n_comp.ctypes.data_as(_IP), modes.ctypes.data_as(_IP), sds.ctypes.data_as(_IP),
        vp([s["bounds"] for s in specs]), ids.ctypes.data_as(_IP), T, betas.ctypes.data_as(_DP), W, int(steps), int(burn), int(swap_every),
        int(seed) & (2 ** 64 - 1), float(a), vp(starts), *[out[k].ctypes.data_as(_DP) for k in
                                                          ("lnZ", "lnZ_se", "lnZ_ti", "mean_lnL", "var_lnL", "move_accept", "swap_accept")],
        vp(chains), vp(chain_ll), 0, None if trace is None else trace.ctypes.data_as(_DP),
        None if swaps is None else swaps.ctypes.data_as(C.POINTER(C.c_uint8))), lib)
    recs = []
    for g in range(G):
        recs.append({"lnZ": float(out["lnZ"][g]), "lnZ_se": float(out["lnZ_se"][g]), "lnZ_ti": float(out["lnZ_ti"][g]), "betas": betas.copy(),
                     "mean_lnL": out["mean_lnL"][g * T:(g + 1) * T].copy(), "var_lnL": out["var_lnL"][g * T:(g + 1) * T].copy(),
                     "move_accept": out["move_accept"][g * T:(g + 1) * T].copy(),
                     "swap_accept": out["swap_accept"][g * (T - 1):(g + 1) * (T - 1)].copy(), "chain": chains[g], "chain_lnl": chain_ll[g],
                     "lnl_trace": None if trace is None else trace[g], "swap_trace": None if swaps is None else swaps[g]})
    return recs


def log_evidence(regions, n_temps=16, walkers=32, steps=600, burn=200, swap_every=5, seed=DEFAULT_SEED, betas=None, start=None, device=0,
                 a=2.0, return_chain=False, trace=False):
    """ln Z of one region (a dict; returns one ``Evidence``) or of a list of regions (returns a list), in one library
    call.  ``betas``: the ladder (increasing from 0 to 1; default: ``default_betas(n_temps)``); ``start``: a [walkers, D]
    block copied to every rung (one region) or a list of such blocks / None per region; None = prior draws.
    ``steps`` full stretch steps per rung, the first ``burn`` dropped, an exchange between neighbouring rungs offered
    after every ``swap_every``."""
    single = isinstance(regions, dict)
    regs = [regions] if single else list(regions)
    if not regs:
        return []
    specs = [_spec(r, i) for i, r in enumerate(regs)]
    if single and start is not None:
        start = [start]
    if start is not None and len(start) != len(specs):
        raise ValueError("one start block (or None) per region is required")
    for sp, s in zip(specs, start or []):
        D = Q_OF_MODE.get(sp["mode"], 3) * sp["n_comp"] + int(sp["sample_sd"])
        if s is not None and np.shape(s) != (int(walkers), D):
            raise ValueError(f"a start block must be [walkers, D] = [{int(walkers)}, {D}]")
    if betas is None:
        betas = default_betas(n_temps)
    recs = [Evidence(**r) for r in _run(specs, np.asarray(betas, dtype=np.float64), walkers, steps, burn, swap_every, seed, a, start, device,
                                        return_chain, trace)]
    for rec, sp in zip(recs, specs):
        rec.n_comp, rec.mode, rec.sample_sd = sp["n_comp"], sp["mode"], bool(sp["sample_sd"])
    return recs[0] if single else recs


def fit_region(fit, region_id=0):
    """the region dict of a ``VPfit`` (device units: ``fit._x``)"""
    return {"x": fit._x, "flux": fit._flux, "noise": None if fit._sample_sd else fit.noise, "n_comp": fit._n, "mode": int(fit._mode),
            "sample_sd": bool(fit._sample_sd), "region_id": int(region_id)}


def fit_start(fit, walkers):
    """a fit's last ensemble as a start block: its first ``walkers`` walkers, or None when it has no chain or fewer"""
    chain = getattr(fit, "_chain_dev", None)
    if chain is None or chain.shape[0] == 0 or chain.shape[1] < int(walkers):
        return None
    return np.ascontiguousarray(chain[-1, :int(walkers)], dtype=np.float64)


def fits_evidence(fits, device=0, **kw):
    """ln Z of the regions of many ``VPfit`` objects in ONE library call; the start is each fit's last ensemble when
    it has one (else prior draws).  Each record is cached as ``fit.evidence``.  Keywords as ``log_evidence``.  Returns
    the records, in the order of ``fits``."""
    fits = list(fits)
    if not fits:
        return []
    walkers = kw.get("walkers", 32)
    recs = log_evidence([fit_region(f, i) for i, f in enumerate(fits)], start=[fit_start(f, walkers) for f in fits], device=device, **kw)
    for f, r in zip(fits, recs):
        f.evidence = r
    return recs
