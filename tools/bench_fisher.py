#!/usr/bin/env python3
"""Cost of the Fisher-matrix library (libvamp_fisher.so) on the shape of a q1422 fit, one JSON line:

  421 groups (the region lengths of tests/golden/q1422_spectrum.npz), 1 .. 4 Voigt lines per region, free sd:
  tools/bench_pred.py's workload; the points are the first walkers of its first kept sample (a 1 % ball about the
  region's centre), ONE point per region -- what VPspectrum.fisher() asks -- and 64 points per region.

  library   one vamp_fisher_points call, HIP events around it, after a warm-up call, --reps repeats: from host points
            with every output but the Jacobian back, and from device-resident points.  The call includes its
            allocations, the upload of the regions and one stream synchronisation
  numpy     the restatement (tests/fisher_ref.py: scipy's wofz, numpy.linalg) on the same points, every
            --ref-every-th region, scaled by the number of points; and how far the two are apart

python tools/bench_fisher.py [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fisher_ref as ref  # noqa: E402
from bench_pred import timed, workload  # noqa: E402
from vamp_amd import fisher  # noqa: E402

WANT = ("grad", "info", "cov", "sigma", "logdet", "chi2", "status")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-every", type=int, default=10)
    ap.add_argument("--library-only", action="store_true")
    a = ap.parse_args()
    xs, fluxes, chains, ks = workload()
    G = len(xs)
    dims = [4 * k + 1 for k in ks]
    out = {"metric": "fisher", "groups": G, "pixels": int(sum(len(x) for x in xs)), "lines": int(sum(ks)),
           "regions_by_K": {str(k): int(np.sum(np.array(ks) == k)) for k in sorted(set(ks))}}
    common = (xs, fluxes, [None] * G, ks, [1] * G, [1] * G)
    for n in (1, 64):
        pts = [np.ascontiguousarray(c[0, :n]) for c in chains]
        tag = "points_%d" % n
        t, flat = timed(lambda: fisher._call(0, *common, [p.ctypes.data for p in pts], False, dims, [n] * G, want=WANT), a.reps)
        out[tag + "_host_points_event_ms"] = t
        tens = [torch.from_numpy(p).to("cuda:0") for p in pts]
        torch.cuda.synchronize()
        t, flat_dev = timed(lambda: fisher._call(0, *common, [v.data_ptr() for v in tens], True, dims, [n] * G, want=WANT), a.reps)
        out[tag + "_device_points_event_ms"] = t
        out[tag + "_device_equals_host_input"] = bool(all(np.array_equal(flat[k], flat_dev[k], equal_nan=True) for k in WANT))
        out[tag + "_status_counts"] = {str(s): int(np.sum(flat["status"] == s)) for s in np.unique(flat["status"])}
        if a.library_only:
            continue
        recs = fisher._split({**flat, "jac": None}, dims, [len(x) for x in xs], [n] * G, False)
        sub = list(range(0, G, a.ref_every))
        t0 = time.perf_counter()
        want = []
        for g in sub:
            for p in pts[g]:
                f, J = ref.jacobian(xs[g], p, ks[g], 1, True)
                want.append(ref.from_jacobian(J, f, fluxes[g], None, p, ks[g], 1))
        t_ref = time.perf_counter() - t0
        out[tag + "_numpy_restatement_ms"] = {"measured_on_regions": len(sub), "measured": t_ref * 1e3, "scaled_to_all": t_ref * 1e3 * G / len(sub)}
        got = [r for g in sub for r in recs[g]]
        # the two against each other where the comparison means something: status 0 and a scaled information of
        # condition number <= 1e6 (numpy inverts the unscaled matrix, and scipy's identity loses the large dampings)
        ok = [(r, w) for r, w in zip(got, want) if r.status == 0 and ref.kappa(w["info"]) <= 1e6]
        with np.errstate(all="ignore"):
            diff = np.array([np.max(np.abs(r.sigma / np.sqrt(np.diag(w["cov"])) - 1.0)) for r, w in ok])
        out[tag + "_sigma_rel_diff_from_restatement"] = {"points_compared": len(ok), "median": float(np.median(diff)), "max": float(np.max(diff))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
