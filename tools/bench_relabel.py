#!/usr/bin/env python3
"""Cost of the relabelling (libvamp_relabel.so) on the shape of a q1422 fit, one JSON line:

  421 groups (the region lengths of tests/golden/q1422_spectrum.npz), W = 64 walkers, N = 180 kept samples (S = 11 520
  per region, 4.85 M assignment problems per round), 1 .. 4 Voigt lines per region, free sd: tools/bench_pred.py's
  workload, with the labels of every second walker permuted at random so that there is something to undo.  The
  reference of a region is its ball's centre, the scale the pooled standard deviations.

  library   one vamp_relabel_chains call, HIP events around it, after a warm-up call, --reps repeats, at max_iter = 1
            and = 10: from device-resident chains (moments and counts back, no chain written; and in place with the
            permutations and costs copied to the host) and from host chains (adds the staging copy, the relabelled
            chain and every output back).  The call includes its allocations and one stream synchronisation per round
  numpy     the restatement (tests/relabel_ref.py: brute force for K <= 6, which is every region here) on every
            --ref-every-th region at max_iter = 1 and = 10, scaled by S K; and scipy's linear_sum_assignment alone on
            the cost matrices of those regions, the figure a Python loop over the samples would pay per round

python tools/bench_relabel.py [--reps 3]"""
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
import relabel_ref as ref  # noqa: E402
from bench_pred import N_KEEP, W, timed, workload  # noqa: E402
from vamp_amd import relabel  # noqa: E402

MOMENTS = ("label_mean", "label_sd", "scale", "n_iter", "n_changed", "n_switched", "n_used", "n_bad")
ALL = ("perm", "cost") + MOMENTS


def switched_workload(seed=1423):
    """bench_pred's chains with the lines of every second walker permuted at random; (chains, K, references)"""
    _, _, chains, ks = workload()
    rng = np.random.default_rng(seed)
    refs = []
    for c, K in zip(chains, ks):
        refs.append(c[:, :, :4 * K].reshape(-1, K, 4).mean(axis=0))
        for w in range(1, W, 2):
            order = rng.permutation(K)
            c[:, w, :4 * K] = c[:, w, :4 * K].reshape(N_KEEP, K, 4)[:, order].reshape(N_KEEP, 4 * K)
    return chains, ks, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-every", type=int, default=40)
    ap.add_argument("--library-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    chains, ks, refs = switched_workload()
    G, S = len(chains), N_KEEP * W
    out = {"metric": "relabel", "groups": G, "S": S, "assignments_per_round": G * S, "lines": int(sum(ks)),
           "regions_by_K": {str(k): int(np.sum(np.array(ks) == k)) for k in sorted(set(ks))}, "chain_bytes": int(sum(c.nbytes for c in chains))}
    ld = [c.shape[1] * c.shape[2] for c in chains]
    common = dict(n_comp=ks, modes=[1] * G, sample_sd=[1] * G, ld=ld, n_keep=[N_KEEP] * G, walkers=[W] * G, refs=refs, scales=None)
    tens = [torch.from_numpy(c).to(dev) for c in chains]
    torch.cuda.synchronize()
    bases = [t.data_ptr() for t in tens]
    host = [c.ctypes.data for c in chains]
    outs = [np.empty_like(c) for c in chains]
    for it in (1, 10):
        tag = "max_iter_%d" % it
        t, flat_dev = timed(lambda: relabel._call(0, bases=bases, is_device=True, max_iter=it, want=MOMENTS, **common), a.reps)
        out[tag + "_device_chains_moments_only_event_ms"] = t
        t, flat_host = timed(lambda: relabel._call(0, bases=host, is_device=False, max_iter=it, outs=[o.ctypes.data for o in outs], out_ld=ld,
                                                   out_is_device=False, want=ALL, **common), a.reps)
        out[tag + "_host_chains_every_output_event_ms"] = t
        cat = lambda v: np.concatenate([np.ravel(e) for e in v]) if isinstance(v, list) else np.asarray(v)
        out[tag + "_host_equals_device_input"] = bool(all(np.array_equal(cat(flat_dev[k]), cat(flat_host[k]), equal_nan=True) for k in MOMENTS))
        n_used = flat_host["n_used"].astype(np.int64)
        out[tag + "_result"] = {"share_of_samples_switched": float(flat_host["n_switched"].sum() / n_used.sum()),
                                "regions_converged": int(np.sum((flat_host["n_changed"] == 0) & (flat_host["n_iter"] > 1))),
                                "rounds_max": int(flat_host["n_iter"].max()), "rounds_mean": float(flat_host["n_iter"].mean())}
    # in place on the device chains, permutations and costs to the host: last, it changes the chains
    scratch = [t.clone() for t in tens]
    torch.cuda.synchronize()
    sb = [t.data_ptr() for t in scratch]
    t, _ = timed(lambda: relabel._call(0, bases=sb, is_device=True, max_iter=10, outs=sb, out_ld=ld, out_is_device=True, want=ALL, **common), a.reps)
    out["max_iter_10_device_chains_in_place_every_output_event_ms"] = t
    del tens, scratch
    torch.cuda.empty_cache()
    if not a.library_only:
        from scipy.optimize import linear_sum_assignment
        sub = list(range(0, G, a.ref_every))
        share = sum(S * ks[i] for i in sub) / float(sum(S * k for k in ks))
        for it in (1, 10):
            t0 = time.perf_counter()
            want = [ref.relabel(chains[i], ks[i], 1, 1, refs[i], None, it) for i in sub]
            t_ref = time.perf_counter() - t0
            out["numpy_restatement_max_iter_%d_ms" % it] = {"measured_on_regions": len(sub), "measured": t_ref * 1e3, "scaled_to_all": t_ref * 1e3 / share}
        same = [bool(np.array_equal(w["perm"], flat_host["perm"][i])) for i, w in zip(sub, want)]
        out["permutations_equal_restatement_regions"] = "%d of %d" % (sum(same), len(sub))
        # scipy per sample, by K: the matrices as separate contiguous arrays (what a Python loop would hand it), a warm-up,
        # then the loop alone; scaled to all samples by the regions' K.  The host's CPU is recorded with it.
        per_call = {}
        for K in sorted(set(ks)):
            C_ = np.concatenate([w["costs"] for i, w in zip(sub, want) if ks[i] == K] or [np.zeros((0, K, K))])[:20000]
            if not len(C_):
                continue
            mats = [np.ascontiguousarray(m) for m in C_]
            for m in mats[:200]:
                linear_sum_assignment(m)
            t0 = time.perf_counter()
            for m in mats:
                linear_sum_assignment(m)
            per_call[K] = (time.perf_counter() - t0) / len(mats)
        cpu = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown") \
            if os.path.exists("/proc/cpuinfo") else "unknown"
        known = [k for k in ks if k in per_call]
        out["scipy_linear_sum_assignment"] = {"host_cpu": cpu, "us_per_call_by_K": {str(k): v * 1e6 for k, v in per_call.items()},
                                              "ms_per_round_scaled_to_all": sum(per_call[k] for k in known) * S * 1e3 * G / max(1, len(known))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
