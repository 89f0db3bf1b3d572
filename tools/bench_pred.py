#!/usr/bin/env python3
"""Cost of the pointwise predictive density (libvamp_pred.so) on the shape of a q1422 fit, one JSON line:

  421 groups (the region lengths of tests/golden/q1422_spectrum.npz), W = 64 walkers, N = 180 kept samples
  (S = 11 520 per region), 1 .. 4 Voigt lines per region, free sd (the form every VPregion fit uses).

  library   one vamp_pred_pointwise call, HIP events around it, after a warm-up call: from device-resident chains
            and from host chains (adds the staging copy of the chains); the call includes its allocations, every
            pass's two kernels, the totals and the copy of the results
  numpy     the restatement (tests/predictive_ref.py) on every --ref-every-th region, scaled by S K P: the only
            yardstick, there was no other way to these numbers before this library

--lib PATH times another build of the library (vamp_amd.build.build_pred(out=..., defines=[...]): the other
orientation of the scratch, the wavefront-only form); --variants times the builds that --build-variants made, in this
process, alternating with the default build.   python tools/bench_pred.py [--reps 5] [--build-variants | --variants]"""
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
import posterior_ref as pref  # noqa: E402
import predictive_ref as ref  # noqa: E402
from vamp_amd import _pred_lib, predictive  # noqa: E402

N_KEEP, W = 180, 64
VARIANTS = {"wavefront_only": ["VAMP_PRED_NARROW=0"], "sample_major": ["VAMP_PRED_PIXEL_MAJOR=0"]}


def variant_path(label):
    return os.path.join(ROOT, "vamp_amd", "libvamp_pred_%s.so" % label)


def workload(seed=1422):
    g = np.load(os.path.join(ROOT, "tests", "golden", "q1422_spectrum.npz"))
    rng = np.random.default_rng(seed)
    xs, fluxes, chains, ks = [], [], [], []
    for s, e in g["region_pixels"]:
        P = int(e - s)
        K = int(rng.choice([1, 1, 2, 3, 4]))
        x = np.arange(P, dtype=np.float64) - 0.5 * (P - 1)
        centre = pref.draw_prior(rng, x, K, 1, 1)[0]
        centre[2::4] += 0.5
        centre[3::4] += 1.0                    # widths of a pixel or more, as a fit's are
        flux = np.exp(-pref.sample_taus(x, centre[None], K, 1)[0].sum(axis=0)) + 0.05 * rng.standard_normal(P)
        xs.append(x); fluxes.append(flux); ks.append(K)
        chains.append(pref.ball(rng, np.append(centre, 0.05), N_KEEP * W).reshape(N_KEEP, W, -1))
    return xs, fluxes, chains, ks


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
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libvamp_pred.so")
    ap.add_argument("--label", default="default")
    ap.add_argument("--ref-every", type=int, default=40)
    ap.add_argument("--library-only", action="store_true")
    ap.add_argument("--variants", action="store_true", help="also time the variant builds (built beforehand by --build-variants)")
    ap.add_argument("--build-variants", action="store_true", help="build the variant libraries and exit (needs no GPU)")
    a = ap.parse_args()
    if a.build_variants:
        import vamp_amd.build as vb
        for label, defines in VARIANTS.items():
            print(vb.build_pred(out=variant_path(label), defines=defines))
        return
    if a.lib:
        _pred_lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda", 0)
    xs, fluxes, chains, ks = workload()
    G = len(xs)
    S = N_KEEP * W
    pix = int(sum(x.size for x in xs))
    evals = int(sum(S * x.size * k for x, k in zip(xs, ks)))
    out = {"metric": "pointwise_predictive", "label": a.label, "groups": G, "S": S, "pixels": pix, "lines": int(sum(ks)),
           "voigt_evaluations": evals, "loglik_matrix_bytes": 8 * S * pix}
    common = dict(noises=[None] * G, n_comp=ks, modes=[1] * G, sample_sd=[1] * G, ld=[c.shape[1] * c.shape[2] for c in chains],
                  n_keep=[N_KEEP] * G, walkers=[W] * G)
    tens = [torch.from_numpy(c).to(dev) for c in chains]
    torch.cuda.synchronize()
    from_dev = lambda: predictive._call(0, xs, fluxes, bases=[t.data_ptr() for t in tens], is_device=True, **common)
    out["device_chains_event_ms"], flat_dev = timed(from_dev, a.reps)
    out["host_chains_event_ms"], flat = timed(lambda: predictive._call(0, xs, fluxes, bases=[c.ctypes.data for c in chains], is_device=False,
                                                                       **common), a.reps)
    out["host_chains_event_ms"]["chain_bytes"] = int(sum(c.nbytes for c in chains))
    out["host_equals_device_input"] = bool(all(np.array_equal(flat[k], flat_dev[k], equal_nan=True) for k in flat))
    if a.variants:
        # A/B in one process, alternating with the default build: each variant is a library of its own name
        default_lib = _pred_lib.load()
        out["variants"] = {}
        for label in VARIANTS:
            lib = _pred_lib.bind(variant_path(label))
            rounds = {"default": [], label: []}
            same = True
            for _ in range(3):
                for name, handle in (("default", default_lib), (label, lib)):
                    _pred_lib.load = lambda h=handle: h
                    t, res = timed(from_dev, a.reps)
                    rounds[name].append(t["median"])
                    same = same and all(np.array_equal(res[k], flat_dev[k], equal_nan=True) for k in res)
            _pred_lib.load = lambda h=default_lib: h
            out["variants"][label] = {"device_chains_event_ms_median_per_round": rounds, "equals_default_bit_for_bit": bool(same)}
    del tens
    torch.cuda.empty_cache()
    if not a.library_only:
        got = predictive._split(flat, [x.size for x in xs], [1] * G)
        sub = list(range(0, G, a.ref_every))
        t0 = time.perf_counter()
        want = [ref.pointwise(xs[i], fluxes[i], None, chains[i], ks[i], 1, True) for i in sub]
        t_ref = time.perf_counter() - t0
        share = sum(S * xs[i].size * ks[i] for i in sub) / evals
        worst = max(ref.check({k: getattr(got[i], k) for k in ref.FLAT}, w, "region %d" % i) for i, w in zip(sub, want))
        out["numpy_restatement_ms"] = {"measured_on_regions": len(sub), "measured": t_ref * 1e3, "scaled_to_all": t_ref * 1e3 / share}
        out["worst_error_over_bar_vs_restatement"] = worst
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
