#!/usr/bin/env python3
"""Cost of PSIS-LOO (libvamp_loo.so) on the shape of a q1422 fit, one JSON line:

  421 groups (the region lengths of tests/golden/q1422_spectrum.npz), W = 64 walkers, N = 180 kept samples
  (S = 11 520 per region, tail length M = 322), 1 .. 4 Voigt lines per region, free sd: tools/bench_pred.py's workload.

  library   one vamp_loo_pointwise call, HIP events around it, after a warm-up call, --reps repeats: from
            device-resident chains and from host chains (adds the staging copy of the chains); the call includes its
            allocations, every pass's two kernels, the totals and the copy of the results
  WAIC      vamp_pred_pointwise on the same chains in the same process, alternating with the LOO call.  The two
            evaluation kernels are the same code, so the difference of the two calls is what the PSIS column stage
            costs over the WAIC column stage
  numpy     the restatement (tests/loo_ref.py) on every --ref-every-th region, scaled by S K P

--lib PATH times another build of libvamp_loo.so (vamp_amd.build.build_loo(out=...)), --label names it in the output:
two builds are compared one process each, in turn.   python tools/bench_loo.py [--reps 3] [--lib PATH --label NAME]"""
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
import loo_ref as ref  # noqa: E402
import predictive_ref  # noqa: E402
from bench_pred import N_KEEP, W, timed, workload  # noqa: E402
from vamp_amd import _loo_lib, loo, predictive  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libvamp_loo.so")
    ap.add_argument("--label", default="default")
    ap.add_argument("--ref-every", type=int, default=40)
    ap.add_argument("--library-only", action="store_true")
    a = ap.parse_args()
    if a.lib:
        _loo_lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda", 0)
    xs, fluxes, chains, ks = workload()
    G = len(xs)
    S = N_KEEP * W
    pix = int(sum(x.size for x in xs))
    evals = int(sum(S * x.size * k for x, k in zip(xs, ks)))
    out = {"metric": "psis_loo", "label": a.label, "groups": G, "S": S, "tail_length": ref.tail_len(S), "pixels": pix, "lines": int(sum(ks)),
           "voigt_evaluations": evals, "loglik_matrix_bytes": 8 * S * pix}
    common = dict(noises=[None] * G, n_comp=ks, modes=[1] * G, sample_sd=[1] * G, ld=[c.shape[1] * c.shape[2] for c in chains],
                  n_keep=[N_KEEP] * G, walkers=[W] * G)
    tens = [torch.from_numpy(c).to(dev) for c in chains]
    torch.cuda.synchronize()
    bases = [t.data_ptr() for t in tens]
    loo_dev = lambda: loo._call(0, xs, fluxes, bases=bases, is_device=True, **common)
    waic_dev = lambda: predictive._call(0, xs, fluxes, bases=bases, is_device=True, **common)
    rounds = {"loo": [], "waic": []}
    for _ in range(3):                          # alternating, as an A/B in one process
        t, flat_dev = timed(loo_dev, a.reps)
        rounds["loo"].append(t["median"])
        t, waic = timed(waic_dev, a.reps)
        rounds["waic"].append(t["median"])
    t_loo, t_waic = float(np.median(rounds["loo"])), float(np.median(rounds["waic"]))
    out["device_chains_event_ms_median_per_round"] = rounds
    out["loo_call_over_waic_call"] = t_loo / t_waic
    out["loo_column_stage_over_waic_call"] = (t_loo - t_waic) / t_waic      # the calls differ by their column stages
    out["lppd_equals_waic_call_bit_for_bit"] = bool(np.array_equal(flat_dev["lppd"], waic["lppd"], equal_nan=True))
    out["host_chains_event_ms"], flat = timed(lambda: loo._call(0, xs, fluxes, bases=[c.ctypes.data for c in chains], is_device=False,
                                                                **common), a.reps)
    out["host_chains_event_ms"]["chain_bytes"] = int(sum(c.nbytes for c in chains))
    out["host_equals_device_input"] = bool(all(np.array_equal(flat[k], flat_dev[k], equal_nan=True) for k in flat))
    k = flat["khat"]
    out["khat"] = {"min": float(np.nanmin(k)), "median": float(np.nanmedian(k)), "max_finite": float(np.max(k[np.isfinite(k)])),
                   "above_0.7": int(np.sum(k > 0.7)), "not_finite": int(np.sum(~np.isfinite(k)))}
    del tens
    torch.cuda.empty_cache()
    if not a.library_only:
        got = loo._split(flat, [x.size for x in xs], [1] * G)
        sub = list(range(0, G, a.ref_every))
        t0 = time.perf_counter()
        want = [ref.pointwise(xs[i], fluxes[i], None, chains[i], ks[i], 1, True) for i in sub]
        t_ref = time.perf_counter() - t0
        share = sum(S * xs[i].size * ks[i] for i in sub) / evals
        out["numpy_restatement_ms"] = {"measured_on_regions": len(sub), "measured": t_ref * 1e3, "scaled_to_all": t_ref * 1e3 / share}
        # the library against the restatement THROUGH the evaluation: lppd at predictive_ref's bars; for the PSIS outputs
        # (whose exact-input bars do not apply here) the worst differences are reported, not asserted
        worst = {"lppd_error_over_bar": 0.0, "khat_abs": 0.0, "elpd_loo_pix_rel": 0.0}
        for i, w in zip(sub, want):
            g = got[i]
            worst["lppd_error_over_bar"] = max(worst["lppd_error_over_bar"], float(np.max(np.abs(g.lppd - w["lppd"]) / predictive_ref.bars(w)["lppd"])))
            fin = np.isfinite(w["khat"])
            worst["khat_abs"] = max(worst["khat_abs"], float(np.max(np.abs(g.khat[fin] - w["khat"][fin]), initial=0.0)))
            worst["elpd_loo_pix_rel"] = max(worst["elpd_loo_pix_rel"], float(np.max(np.abs(g.elpd_loo_pix - w["elpd_loo_pix"]) /
                                                                                     np.maximum(1.0, np.abs(w["elpd_loo_pix"])))))
        out["worst_vs_restatement"] = worst
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
