#!/usr/bin/env python3
"""Cost of the posterior summaries (libvamp_post.so) on the shape of a q1422 fit, one JSON line:

  421 groups (the region lengths of tests/golden/q1422_spectrum.npz), W = 64 walkers, N = 180 kept samples
  (S = 11 520 per region), 1 .. 4 Voigt lines per region, five probabilities.

  library   one vamp_post_summaries call, HIP events around it, after a warm-up call: from device-resident chains
            and from host chains (adds the staging copy of the chains); the call includes its allocations, every
            pass's two kernels and the copy of the results
  numpy     the restatement (tests/posterior_ref.py) on every --ref-every-th region, scaled by S K P
  loop      the only way before this library: one HipContext.model call per sample, on --loop-regions regions and
            --loop-samples samples each, scaled to every sample of every region

--lib PATH times another build of the library (vamp_amd.build.build_post(out=..., defines=[...]): the other
orientation of the scratch, the wavefront-only form).   python tools/bench_post.py [--reps 5]"""
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
import posterior_ref as ref  # noqa: E402
import vamp_amd  # noqa: E402
from vamp_amd import _post_lib, posterior  # noqa: E402

PROBS = np.asarray(posterior.DEFAULT_PROBS)
N_KEEP, W = 180, 64


def workload(seed=1422):
    g = np.load(os.path.join(ROOT, "tests", "golden", "q1422_spectrum.npz"))
    rng = np.random.default_rng(seed)
    xs, chains, ks = [], [], []
    for s, e in g["region_pixels"]:
        P = int(e - s)
        K = int(rng.choice([1, 1, 2, 3, 4]))
        x = np.arange(P, dtype=np.float64) - 0.5 * (P - 1)
        centre = ref.draw_prior(rng, x, K, 1, 1)[0]
        centre[2::4] += 0.5
        centre[3::4] += 1.0                    # widths of a pixel or more, as a fit's are
        xs.append(x); ks.append(K)
        chains.append(ref.ball(rng, centre, N_KEEP * W).reshape(N_KEEP, W, -1))
    return xs, chains, ks


def timed(fn, reps):
    fn()                                        # warm-up: code object load, the LDS attribute
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libvamp_post.so")
    ap.add_argument("--label", default="default")
    ap.add_argument("--ref-every", type=int, default=40)
    ap.add_argument("--loop-regions", type=int, default=4)
    ap.add_argument("--loop-samples", type=int, default=256)
    ap.add_argument("--library-only", action="store_true")
    a = ap.parse_args()
    if a.lib:
        _post_lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda", 0)
    xs, chains, ks = workload()
    G = len(xs)
    S = N_KEEP * W
    pix = int(sum(x.size for x in xs))
    evals = int(sum(S * x.size * k for x, k in zip(xs, ks)))
    out = {"metric": "posterior_summaries", "label": a.label, "groups": G, "S": S, "pixels": pix, "lines": int(sum(ks)),
           "voigt_evaluations": evals, "flux_matrix_bytes": 8 * S * pix}
    common = dict(n_comp=ks, modes=[1] * G, sample_sd=[0] * G, ld=[c.shape[1] * c.shape[2] for c in chains], n_keep=[N_KEEP] * G,
                  walkers=[W] * G, widths=[1.0] * G, probs=PROBS)
    tens = [torch.from_numpy(c).to(dev) for c in chains]
    torch.cuda.synchronize()
    med, best, flat_dev = timed(lambda: posterior._call(0, xs, bases=[t.data_ptr() for t in tens], is_device=True, **common), a.reps)
    out["device_chains_event_ms"] = {"median": med, "min": best}
    med, best, flat = timed(lambda: posterior._call(0, xs, bases=[c.ctypes.data for c in chains], is_device=False, **common), a.reps)
    out["host_chains_event_ms"] = {"median": med, "min": best, "chain_bytes": int(sum(c.nbytes for c in chains))}
    out["host_equals_device_input"] = bool(all(np.array_equal(flat[k], flat_dev[k], equal_nan=True) for k in flat))
    del tens
    torch.cuda.empty_cache()
    if not a.library_only:
        got = posterior._split(flat, [x.size for x in xs], ks, PROBS, [1] * G)
        # the restatement on a subset, scaled by its share of the evaluations
        sub = list(range(0, G, a.ref_every))
        t0 = time.perf_counter()
        want = [ref.summaries(xs[i], chains[i], ks[i], 1, probs=PROBS) for i in sub]
        t_ref = time.perf_counter() - t0
        share = sum(S * xs[i].size * ks[i] for i in sub) / evals
        err_f = max(float(np.max(np.abs(got[i].flux_q - w["flux_q"]))) for i, w in zip(sub, want))
        err_e = max(float(np.max(np.abs(got[i].ew_q - w["ew_q"])) / xs[i].size) for i, w in zip(sub, want))
        out["numpy_restatement_ms"] = {"measured_on_regions": len(sub), "measured": t_ref * 1e3, "scaled_to_all": t_ref * 1e3 / share}
        out["max_abs_flux_q_diff_vs_restatement"] = err_f
        out["max_abs_ew_q_diff_per_pixel_vs_restatement"] = err_e
        # one vamp_model launch per sample
        pick = list(range(0, G, max(1, G // a.loop_regions)))[:a.loop_regions]
        t_loop, n_loop = 0.0, 0
        for i in pick:
            th = chains[i].reshape(S, -1)[:a.loop_samples]
            with vamp_amd.HipContext(device=0) as ctx:
                ctx.set_regions(xs[i], np.ones_like(xs[i]), np.ones_like(xs[i]), ks[i], mode=vamp_amd.MODE_VOIGT4)
                ctx.model(th[0])
                t0 = time.perf_counter()
                for t in th:
                    ctx.model(t)
                t_loop += time.perf_counter() - t0
                n_loop += len(th)
        per = t_loop / n_loop
        out["model_call_per_sample"] = {"regions": len(pick), "samples_each": a.loop_samples, "ms_per_call": per * 1e3,
                                        "scaled_to_all_ms": per * 1e3 * S * G, "note": "evaluation only: the statistics would still be numpy's"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
