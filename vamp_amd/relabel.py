"""Undo label switching on the GPU: the K lines of a region are exchangeable, so a walker may sit in any of the K!
copies of a posterior mode, and a per-line mean, standard deviation, R-hat or autocorrelation time taken per parameter
slot mixes lines.  For every sample the library finds the permutation of its lines that lies closest to a reference
labelling, moves the reference to the relabelled means, and repeats until nothing changes (libvamp_relabel.so,
include/vamp_relabel.h; definitions: DESIGN.md "Relabelling: undoing label switching").

    relabel_chains(chains, n_comp, modes, sample_sd, refs, scales=None, max_iter=10)     host [N, W, D] arrays
    context_relabel(ctx, chain_ptr, n_keep, refs, ..., in_place=False)                   the device chain HipContext.run_dev wrote
    fits_relabel(fits, max_iter=10)                                                      the chains of many VPfit objects
    assign(cost)                                                                         the solver alone, on [n, K, K] cost matrices

Each call is ONE library call for all the arrays / regions it is given.  Chains and references are in the same units
(a fit's device units: ``fit._chain_dev`` and ``fit._theta_dev``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _relabel_lib
from ._sidelib import Q_OF_MODE, check_chain_shapes, context_layout, fits_with_chain, host_layout, per_group

MAX_COMPONENTS = 32           # VAMP_RELABEL_MAX_COMPONENTS of include/vamp_relabel.h
DEFAULT_MAX_ITER = 10         # rounds of every entry point below; what stats / trace / diagnostics(relabel=True) of a fit read

_COUNTS = ("n_iter", "n_changed", "n_switched", "n_used", "n_bad")


class RelabelRecord:
    """The relabelling of one region's ensemble: ``perm`` [N, W, K] uint8 (label j of sample (t, w) is its line
    perm[t, w, j]), ``cost`` [N, W] (the attained distance; NaN for a bad sample), ``label_mean`` and ``label_sd``
    [K, q] over the ``n_used`` good samples, ``scale`` [q], the counts ``n_iter``, ``n_changed`` (of the last round),
    ``n_switched``, ``n_used``, ``n_bad``, ``converged`` (the last of at least two rounds changed nothing) and ``chain``
    ([N, W, D], the relabelled chain, or None when it was not asked for)."""

    __slots__ = ("perm", "cost", "label_mean", "label_sd", "scale", "chain", "converged", "max_iter") + _COUNTS

    def __init__(self, perm, cost, label_mean, label_sd, scale, n_iter, n_changed, n_switched, n_used, n_bad, chain=None, max_iter=None):
        self.perm, self.cost, self.label_mean, self.label_sd, self.scale, self.chain = perm, cost, label_mean, label_sd, scale, chain
        self.n_iter, self.n_changed, self.n_switched, self.n_used, self.n_bad = (int(v) for v in (n_iter, n_changed, n_switched, n_used, n_bad))
        self.converged = self.n_changed == 0 and self.n_iter > 1
        self.max_iter = max_iter

    def gather(self, chain):
        """``chain`` [N, W, D'] (any units; D' >= q K) with line j <- line perm[t, w, j]; what follows the lines stays"""
        chain = np.asarray(chain)
        N, W, K = self.perm.shape
        q = self.label_mean.shape[1]
        out = chain.reshape(N, W, -1).copy()
        v = out[:, :, :q * K].reshape(N, W, K, q)
        out[:, :, :q * K] = np.take_along_axis(v, self.perm[..., None].astype(np.intp), axis=2).reshape(N, W, q * K)
        return out.reshape(chain.shape)

    def __repr__(self):
        return (f"RelabelRecord(shape={self.perm.shape}, n_iter={self.n_iter}, converged={self.converged}, n_switched={self.n_switched}, "
                f"n_changed={self.n_changed}, n_used={self.n_used}, n_bad={self.n_bad})")


def _call(device, n_comp, modes, sample_sd, bases, is_device, ld, n_keep, walkers, refs, scales, max_iter, outs=None, out_ld=None,
          out_is_device=False, stream=None, want=("perm", "cost", "label_mean", "label_sd", "scale") + _COUNTS):
    """One vamp_relabel_chains call; returns the outputs asked for by name: per group ``perm`` [S, K], ``cost`` [S],
    ``label_mean`` / ``label_sd`` [K, q], ``scale`` [q]; the counts as [G] int32 arrays.  ``outs``: None, or per group
    None or the address the relabelled chain goes to (``out_ld`` doubles between its rows)."""
    lib = _relabel_lib.load()
    G = len(bases)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    ptrs = lambda addrs: (C.c_void_p * G)(*[None if a is None else int(a) for a in addrs])
    qs = [Q_OF_MODE.get(int(m), 3) for m in modes]
    S = [int(n) * int(w) for n, w in zip(n_keep, walkers)]
    refs = [np.ascontiguousarray(r, dtype=np.float64) for r in refs]
    for r, k, q in zip(refs, n_comp, qs):
        if r.size != int(k) * q:
            raise ValueError(f"a reference of {r.size} values does not hold {k} lines of {q} parameters")
    scales = [None] * G if scales is None else [None if s is None else np.ascontiguousarray(s, dtype=np.float64) for s in scales]
    for s, q in zip(scales, qs):
        if s is not None and s.shape != (q,):
            raise ValueError("a scale holds one value per parameter of a line")
    out = {}
    if "perm" in want:
        out["perm"] = [np.empty((s, int(k)), dtype=np.uint8) for s, k in zip(S, n_comp)]
    if "cost" in want:
        out["cost"] = [np.empty(s) for s in S]
    n_col, n_sc = sum(int(k) * q for k, q in zip(n_comp, qs)), sum(qs)
    flat = {k: np.empty(n) for k, n in (("label_mean", n_col), ("label_sd", n_col), ("scale", n_sc)) if k in want}
    counts = {k: np.empty(G, dtype=np.int32) for k in _COUNTS if k in want}
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _relabel_lib.check(lib.vamp_relabel_chains(
        int(device), C.c_void_p(stream or 0), G, i32(n_comp), i32(modes), i32(sample_sd), ptrs(bases), int(bool(is_device)), i64(ld),
        i32(n_keep), i32(walkers), ptrs([r.ctypes.data for r in refs]),
        None if all(s is None for s in scales) else ptrs([None if s is None else s.ctypes.data for s in scales]), int(max_iter),
        None if outs is None else ptrs(outs), None if outs is None else i64(out_ld), int(bool(out_is_device)),
        ptrs([a.ctypes.data for a in out["perm"]]) if "perm" in out else None,
        ptrs([a.ctypes.data for a in out["cost"]]) if "cost" in out else None,
        *[flat[k].ctypes.data_as(dp) if k in flat else None for k in ("label_mean", "label_sd", "scale")],
        *[counts[k].ctypes.data_as(ip) if k in counts else None for k in _COUNTS]), lib)
    oc = os_ = 0
    for k, q in zip(n_comp, qs):
        n = int(k) * q
        for name in ("label_mean", "label_sd"):
            if name in flat:
                out.setdefault(name, []).append(flat[name][oc:oc + n].reshape(int(k), q).copy())
        if "scale" in flat:
            out.setdefault("scale", []).append(flat["scale"][os_:os_ + q].copy())
        oc, os_ = oc + n, os_ + q
    out.update(counts)
    return out


def _per_chain(flat, G, chains=None):
    """the outputs of ``_call`` as one dict per group"""
    return [dict({k: flat[k][g] for k in flat}, chain=None if chains is None else chains[g]) for g in range(G)]


def _relabel_host(arrays, n_comp, modes, sds, refs, scales, max_iter, device, want_chain):
    """the library call for contiguous fp64 [N, W, D] host arrays; one dict of outputs per array (tests put the numpy
    restatement here)"""
    bases, ld, n_keep, walkers = host_layout(arrays, [1] * len(arrays))
    outs = [np.empty_like(a) for a in arrays] if want_chain else None
    flat = _call(device, n_comp, modes, sds, bases, False, ld, n_keep, walkers, refs, scales, max_iter,
                 None if outs is None else [o.ctypes.data for o in outs], ld, False)
    return _per_chain(flat, len(arrays), outs)


def _records(per_chain, shapes, max_iter):
    return [RelabelRecord(r["perm"].reshape(N, W, -1), r["cost"].reshape(N, W), r["label_mean"], r["label_sd"], r["scale"],
                          *[r[k] for k in _COUNTS], chain=r["chain"], max_iter=max_iter) for r, (N, W) in zip(per_chain, shapes)]


def relabel_chains(chains, n_comp, modes, sample_sd, refs, scales=None, max_iter=DEFAULT_MAX_ITER, device=0, return_chain=False):
    """Records of one host [N, W, D] chain (returns one ``RelabelRecord``) or of a list of chains (returns a list), all
    in one library call.  ``n_comp``, ``modes`` (0 = GAUSS3, 1 = VOIGT4) and ``sample_sd`` (is the last dimension the
    free sd?) are one value for all chains or one per chain; ``refs``: the [K, q] reference labelling of every chain,
    in the chain's units; ``scales``: None (every chain's pooled standard deviations), or per chain None or [q];
    ``return_chain``: the records also hold the relabelled chain."""
    single = isinstance(chains, np.ndarray)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in ([chains] if single else chains)]
    G = len(arrays)
    if G == 0:
        return []
    refs = [refs] if single else list(refs)
    scales = [None] * G if scales is None else ([scales] if single else list(scales))
    if not len(refs) == len(scales) == G:
        raise ValueError("one reference (and one scale or None) per chain are required")
    n_comp, modes, sds = per_group(n_comp, G, int), per_group(modes, G, int), per_group(sample_sd, G, int)
    check_chain_shapes(arrays, n_comp, modes, sds, [f"free sd = {bool(sd)}" for sd in sds])
    recs = _records(_relabel_host(arrays, n_comp, modes, sds, refs, scales, int(max_iter), int(device), bool(return_chain)),
                    [a.shape[:2] for a in arrays], int(max_iter))
    return recs[0] if single else recs


def context_relabel(ctx, chain_ptr, n_keep, refs, scales=None, max_iter=DEFAULT_MAX_ITER, in_place=False):
    """Records of every region of the DEVICE chain ``HipContext.run_dev`` wrote at ``chain_ptr`` ([n_keep, total_theta]
    fp64), one per region, from one library call on the context's device (default stream, after the context's stream
    is synchronised).  ``refs``: one [K, q] reference per region; ``in_place``: the device chain itself is relabelled
    (what a later posterior, predictive or diagnostics call on it then reads)."""
    ctx.synchronize()                  # the sampler's stream is done with the chain before the default stream reads it
    R = len(ctx.ndims)
    if len(refs) != R or (scales is not None and len(scales) != R):
        raise ValueError("one reference (and one scale or None) per region of the context are required")
    ks, modes, sds, bases, ld, n_keep, walkers = context_layout(ctx, chain_ptr, n_keep)
    flat = _call(ctx.device, ks, modes, sds, bases, True, ld, n_keep, walkers, refs, scales, max_iter,
                 bases if in_place else None, ld, True)
    return _records(_per_chain(flat, R), list(zip(n_keep, walkers)), int(max_iter))


def fit_reference(fit):
    """a fit's reference labelling [K, q]: its current point in device units (the MAP, when ``map_estimate`` ran)"""
    K, q = int(fit._n), Q_OF_MODE[int(fit._mode)]
    return np.asarray(fit._theta_dev, dtype=np.float64)[:K * q].reshape(K, q).copy()


def fits_relabel(fits, max_iter=DEFAULT_MAX_ITER, device=0):
    """Records of the chains of many ``VPfit`` objects in ONE library call; each fit's ``mcmc.relabel()`` cache is filled
    from it.  The reference of a fit is ``fit_reference(fit)``, the scale its chain's pooled standard deviations.  Fits
    without a chain are left out.  Returns (fits relabelled, their records)."""
    have = fits_with_chain(fits)
    if not have:
        return [], []
    recs = relabel_chains([f._chain_dev for f in have], [f._n for f in have], [int(f._mode) for f in have],
                          [int(bool(f._sample_sd)) for f in have], [fit_reference(f) for f in have], max_iter=max_iter, device=device)
    for f, r in zip(have, recs):
        f.mcmc._set_relabel(r)
    return have, recs


def assign(cost, device=0):
    """(perm [n, K] uint8, total [n]) of [n, K, K] cost matrices, cost[m, i, j] = what it costs to give label j to line i:
    the solver of the chain kernel alone (vamp_relabel_assign, a test hook).  A matrix with an entry that is not finite
    gets the identity and total NaN."""
    lib = _relabel_lib.load()
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    if cost.ndim != 3 or cost.shape[1] != cost.shape[2]:
        raise ValueError("cost must be [n, K, K]")
    n, K = cost.shape[:2]
    perm, total = np.empty((n, K), dtype=np.uint8), np.empty(n)
    _relabel_lib.check(lib.vamp_relabel_assign(int(device), K, n, cost.ctypes.data_as(C.POINTER(C.c_double)),
                                               perm.ctypes.data_as(C.POINTER(C.c_uint8)), total.ctypes.data_as(C.POINTER(C.c_double))), lib)
    return perm, total
