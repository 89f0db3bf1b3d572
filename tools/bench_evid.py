#!/usr/bin/env python3
"""Cost of the log-evidence (libvamp_evid.so) on the shape of a q1422 fit, one JSON line:

  421 regions (the region lengths of tests/golden/q1422_spectrum.npz), 1 .. 4 Voigt lines per region, known noise,
  the defaults of vamp_amd.evidence.log_evidence: T = 16 rungs, W = 32 walkers, 600 steps (200 dropped), an exchange
  offered every 5 steps, prior-drawn starts.

  library   one vamp_evid_run call, HIP events around it, after a warm-up call; the call includes its allocations,
            the upload of the regions, every launch and the copy of the results
  numpy     the restatement (tests/evidence_ref.py): --ref-steps steps of ONE region of the median (pixels x lines) on
            one thread, scaled to the call by steps and by the regions' share of pixels x lines x parameters-free
            work (P K); and the same region once per host thread at the same time (processes forked before the GPU is
            touched), scaled the same way -- what all host threads together would need

--lib PATH times another build of the library (vamp_amd.build.build_evid(out=..., defines=["VAMP_EVID_NARROW=0"]):
wavefront-only movers).   python tools/bench_evid.py [--reps 3]"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import evidence_ref as ref  # noqa: E402
from oracle import vamp_oracle as vo  # noqa: E402
from vamp_amd import _evid_lib, evidence  # noqa: E402

T, W, STEPS, BURN, SWAP, SEED = 16, 32, 600, 200, 5, 1422


def workload(seed=1422):
    g = np.load(os.path.join(ROOT, "tests", "golden", "q1422_spectrum.npz"))
    rng = np.random.default_rng(seed)
    regs = []
    for i, (s, e) in enumerate(g["region_pixels"]):
        P = int(e - s)
        K = int(rng.choice([1, 1, 2, 3, 4]))
        x = np.arange(P, dtype=np.float64) - 0.5 * (P - 1)
        tau = sum(vo.voigt_function(x, rng.uniform(x[0], x[-1]), rng.uniform(0.3, 2.0), rng.uniform(0.5, 2.0), rng.uniform(1.5, 4.0))
                  for _ in range(K))
        regs.append({"x": x, "flux": np.exp(-tau) + 0.05 * rng.standard_normal(P), "noise": np.full(P, 0.05), "n_comp": K, "mode": 1,
                     "region_id": i})
    return regs


def _ref_steps(args):
    reg, steps = args
    R = ref.make_region(reg["x"], reg["flux"], reg["noise"], reg["n_comp"], reg["mode"])
    t0 = time.perf_counter()
    out = ref.run([R], [reg["region_id"]], ref.default_betas(T), W, steps, 0, SWAP, SEED)[0]
    return time.perf_counter() - t0, out


def timed(fn, reps):
    fn()                                        # warm-up: code object load
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libvamp_evid.so")
    ap.add_argument("--label", default="default")
    ap.add_argument("--ref-steps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1))
    ap.add_argument("--library-only", action="store_true")
    a = ap.parse_args()
    if a.lib:
        _evid_lib.LIB_PATH = os.path.abspath(a.lib)
    regs = workload()
    G = len(regs)
    work = np.array([r["x"].size * r["n_comp"] for r in regs], dtype=np.float64)
    out = {"metric": "log_evidence", "label": a.label, "regions": G, "n_temps": T, "walkers": W, "steps": STEPS, "burn": BURN,
           "swap_every": SWAP, "pixels": int(sum(r["x"].size for r in regs)), "lines": int(sum(r["n_comp"] for r in regs)),
           "narrow_regions": int(sum(r["x"].size <= 32 and r["n_comp"] <= 4 for r in regs))}
    ref_out = None
    if not a.library_only:          # the host measurements first: the processes are forked before the GPU is touched
        pick = int(np.argsort(work)[G // 2])
        scale = (STEPS / a.ref_steps) * (work.sum() / work[pick])
        t_one, ref_out = _ref_steps((regs[pick], a.ref_steps))
        with multiprocessing.get_context("fork").Pool(a.threads) as pool:
            t0 = time.perf_counter()
            pool.map(_ref_steps, [(regs[pick], a.ref_steps)] * a.threads)
            t_all = (time.perf_counter() - t0) / a.threads
        out["numpy_restatement_ms"] = {"region": pick, "pixels": int(regs[pick]["x"].size), "lines": regs[pick]["n_comp"], "steps": a.ref_steps,
                                       "measured_one_thread": t_one * 1e3, "one_thread_scaled_to_the_call": t_one * 1e3 * scale,
                                       "threads": a.threads, "all_threads_scaled_to_the_call": t_all * 1e3 * scale}
    torch.cuda.synchronize()
    run = lambda: evidence.log_evidence(regs, n_temps=T, walkers=W, steps=STEPS, burn=BURN, swap_every=SWAP, seed=SEED)
    med, best, recs = timed(run, a.reps)
    out["call_event_ms"] = {"median": med, "min": best}
    out["region_rung_walker_steps_per_second"] = G * T * W * STEPS / (med * 1e-3)
    lnz, se = np.array([r.lnZ for r in recs]), np.array([r.lnZ_se for r in recs])
    out["lnZ_finite"] = int(np.isfinite(lnz).sum())
    out["lnZ_se"] = {"median": float(np.median(se)), "max": float(np.max(se))}
    out["move_accept_beta1_median"] = float(np.median([r.move_accept[-1] for r in recs]))
    out["swap_accept_median"] = float(np.median([np.median(r.swap_accept) for r in recs]))
    if ref_out is not None:         # the same region, the same few steps, on the device: the trajectories agree
        got = evidence.log_evidence(regs[pick], n_temps=T, walkers=W, steps=a.ref_steps, burn=0, swap_every=SWAP, seed=SEED, trace=True)
        out["max_rel_lnL_diff_vs_restatement"] = float(np.max(np.abs(got.lnl_trace - ref_out["lnl_trace"]) / np.maximum(1.0, np.abs(ref_out["lnl_trace"]))))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
