#!/usr/bin/env python3
"""Cost of the regularised metric (libvamp_metric.so) on the shape of a q1422 fit, one JSON line.  Workloads:

  q1422        421 matrices, one per region of tests/golden/q1422_spectrum.npz, D = 4 K + 1 (Voigt lines and the free sd)
               with K the number of lines of tests/golden/q1422_vpm.npz that fall in the region (1 .. 16)
  q1422_x64    64 matrices per region: 26 944 matrices in 421 groups
  d65          421 matrices at D = 65

The matrices are synthetic informations in prior units: a random orthogonal basis and eigenvalues 10^U(-6, 8), so that
about four in ten lie below lam_lo = 1 (no fit is run here: what is timed is the decomposition, whatever the matrix).

  library   one vamp_metric_factor call, HIP events around it, the median of --reps after a warm-up call, from host
            matrices (the call then includes their copy to the device) and from device matrices; every output fetched
  numpy     the same outputs from numpy.linalg.eigh and numpy.linalg.cholesky per matrix, wall clock

--convergence measures, and gates nothing: on tools/bench_hmc.py's quadrature case and four-line Voigt blend, ``fits_hmc``
at its default budget with metric="regularised" and -- after the stretch move's default run -- with metric="chain":
n_low, n_high, the tuned eps, acceptance, walls, worst split-R-hat and least n_eff, beside the stretch move's own figures.

    python tools/bench_metric.py [--reps 5] [--convergence] [--only q1422]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 1422


def line_counts():
    """lines of q1422_vpm.npz per region of q1422_spectrum.npz, clipped to 1 .. 16"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "q1422_spectrum.npz"))
    wl = g["wavelength_milli"] * 1e-3
    lines = np.load(os.path.join(ROOT, "tests", "golden", "q1422_vpm.npz"))["wavelength"]
    ks = []
    for s, e in g["region_pixels"]:
        lo, hi = sorted((wl[s], wl[e - 1]))
        ks.append(int(np.clip(np.sum((lines >= lo) & (lines <= hi)), 1, 16)))
    return ks


def matrices(dims, per_group, seed=SEED):
    rng = np.random.default_rng(seed)
    out = []
    for D in dims:
        q = np.linalg.qr(rng.standard_normal((D, D)))[0]
        grp = np.empty((per_group, D, D))
        for m in range(per_group):
            e = 10.0 ** rng.uniform(-6.0, 8.0, D)
            b = (q * e) @ q.T
            grp[m] = 0.5 * (b + b.T)
        out.append(grp)
    return out


def timed(fn, reps):
    import torch
    fn()                                        # warm-up: code object load, the raised LDS limit
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}, res


def numpy_metric(mats, lam_lo=1.0, lam_hi=2.0 ** 40):
    n_low = 0
    for grp in mats:
        for b in grp:
            e, v = np.linalg.eigh(b)
            n_low += int(np.sum(e < lam_lo))
            lt = np.clip(e, lam_lo, lam_hi)
            cov = (v / lt) @ v.T
            (v * lt) @ v.T
            np.linalg.cholesky(0.5 * (cov + cov.T))
            np.sum(np.log(lt))
    return n_low


def workload_row(name, dims, per_group, reps):
    import torch
    from vamp_amd import metric
    mats = matrices(dims, per_group)
    G = len(mats)
    scales = [np.ones(D) for D in dims]
    n_mats = [per_group] * G
    args = (scales, [0] * G, [1.0] * G, [2.0 ** 40] * G, metric.DEFAULT_SWEEPS)
    row = {"groups": G, "matrices": G * per_group, "dims": {"min": int(min(dims)), "median": float(np.median(dims)), "max": int(max(dims))},
           "matrix_doubles": int(sum(per_group * D * D for D in dims)), "matrices_per_workgroup": metric.plan(max(dims))[0]}
    row["host_matrices_event_ms"], flat = timed(lambda: metric._call(0, mats, dims, dims, n_mats, *args), reps)
    dev = [torch.tensor(m, dtype=torch.float64, device="cuda:0").contiguous() for m in mats]
    torch.cuda.synchronize()
    row["device_matrices_event_ms"], flat_d = timed(lambda: metric._call(0, [t.data_ptr() for t in dev], dims, dims, n_mats, *args, is_device=True), reps)
    row["device_equals_host_bits"] = bool(all(np.array_equal(flat[k], flat_d[k], equal_nan=True) for k in flat))
    row["status_counts"] = {str(s): int(np.sum(flat["status"] == s)) for s in range(4)}
    row["sweeps_used"] = {"median": float(np.median(flat["sweeps_used"])), "max": int(flat["sweeps_used"].max())}
    row["n_low_total"] = int(flat["n_low"].sum())
    t0 = time.perf_counter()
    n_low = numpy_metric(mats)
    row["numpy_eigh_ms"] = (time.perf_counter() - t0) * 1e3
    row["numpy_n_low_total"] = n_low
    return row


def convergence():
    import evidence_ref
    from oracle import vamp_oracle as vo
    from vamp_amd.vpfits import VPfit
    out = {}
    x, flux, noise = evidence_ref.gauss_line_data(24, [(1.2, 11.3, 2.5)], 0.1, 3)
    xb = np.arange(64.0)
    truth = np.array([[0.9, 24.0, 1.0, 4.0], [1.4, 29.0, 0.8, 3.5], [0.7, 35.0, 1.2, 4.5], [1.1, 40.0, 0.6, 3.0]]).ravel()
    R = vo.Region(x=xb, flux=np.ones(64), noise=np.ones(64), n_comp=4, mode=1)
    fb = vo.model_flux(R, truth) + 0.03 * np.random.default_rng(9).standard_normal(64)

    def hmc_row(fit, which):
        t0 = time.perf_counter()
        rec = fit.hmc(metric=which)
        secs = time.perf_counter() - t0
        d = rec.diagnostics() if rec.status == 0 else None
        return {"status": int(rec.status), "seconds": secs, "n_low": rec.n_low, "n_high": rec.n_high, "eps": rec.eps, "n_steps": rec.n_steps,
                "n_leap": rec.n_leap, "accept_rate": None if rec.status else float(np.nanmean(rec.accept_rate)),
                "n_wall": None if rec.status else int(np.sum(rec.n_wall)),
                "max_r_hat": None if d is None else float(np.nanmax(d.r_hat)), "min_n_eff": None if d is None else float(np.nanmin(d.n_eff)),
                "tau_reliable": None if d is None else bool(np.all(d.reliable))}

    for name, (xx, ff, nn, K, voigt) in {"quadrature_one_gauss_line": (x, flux, noise, 1, False),
                                         "four_line_voigt_blend": (xb, fb, np.full(64, 0.03), 4, True)}.items():
        fit = VPfit(noise=nn, seed=5)
        fit.initialise_model(1.0e3 + 2.0 * xx, ff, K, voigt=voigt)
        fit.map_estimate()
        point = np.array(fit._theta_dev)
        row = {"hmc_fisher_status": int(fit.hmc().status), "hmc_regularised": hmc_row(fit, "regularised")}
        t0 = time.perf_counter()
        fit.mcmc_fit(iterations=3000, burnin=300, thinning=15)
        dm = fit.mcmc.diagnostics()
        row["stretch_move"] = {"seconds": time.perf_counter() - t0, "max_r_hat": float(np.nanmax([v["r_hat"] for v in dm.values()])),
                               "min_n_eff": float(np.nanmin([v["n_eff"] for v in dm.values()])),
                               "tau_reliable": bool(all(v["reliable"] for v in dm.values()))}
        row["point_moved_by_the_stretch_run"] = bool(not np.array_equal(point, np.asarray(fit._theta_dev)))
        row["hmc_chain"] = hmc_row(fit, "chain")
        out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one workload: q1422, q1422_x64 or d65")
    ap.add_argument("--convergence", action="store_true", help="also run fits_hmc with the regularised and the chain metric on two cases")
    a = ap.parse_args()
    import torch
    from vamp_amd import metric
    torch.zeros(1, device="cuda:0")
    ks = line_counts()
    dims = [4 * k + 1 for k in ks]
    loads = {"q1422": (dims, 1), "q1422_x64": (dims, 64), "d65": ([65] * len(dims), 1)}
    out = {"metric": "metric_factor", "n_sweeps": metric.DEFAULT_SWEEPS, "lines_per_region": {"min": min(ks), "median": float(np.median(ks)), "max": max(ks)}}
    for name, (d, per) in loads.items():
        if a.only in (None, name):
            out[name] = workload_row(name, d, per, a.reps)
    if a.convergence:
        out["convergence"] = convergence()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
