#!/usr/bin/env python3
"""Cost of the chain diagnostics (libvamp_diag.so) on two shapes, one JSON line:

  q1422    the kept fits of a q1422 spectrum: 421 regions, 64 walkers, N = 180 kept samples, D = 4 or 7
  headline one ensemble of W = 65 536 walkers, D = 48, N = 100 (device-generated AR(1), 2.5 GB); and the same work
           as 48 one-parameter groups, whose staging reads are coalesced (the cost of the stride-D gather)

Per shape: the time of one library call from HIP events around it (device-resident input, after warm-up;
the call includes its scratch allocation, the two kernels and the copy of the results), the wall time of a
call on host arrays (adds the staging copy), the numpy restatement's host time (tests/chain_diag_ref.py;
for the headline measured on a slice of the walkers and scaled by the walker count), the FMAs of the lag sums
(sum W N (N+1)/2 D) and bytes read (8 sum N W D), and the fractions of the fp64 VALU rate (39.3 T lane-ops/s)
and of 8 TB/s these imply at the event time.

--lib PATH times another build of the library (an earlier commit's, to compare the whole call: at the q1422 shape it
is bound by its host side).   python tools/bench_diag.py [--reps 5]"""
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
import chain_diag_ref as ref  # noqa: E402
from vamp_amd import _diag_lib, diagnostics  # noqa: E402

VALU_FP64 = 39.3e12
HBM = 8.0e12


def device_ar1(shape, rho, seed, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    N = shape[0]
    x = torch.empty(shape, dtype=torch.float64, device=dev)
    x[0] = torch.randn(shape[1:], dtype=torch.float64, device=dev, generator=gen) / np.sqrt(1 - rho * rho)
    for t in range(1, N):
        x[t] = rho * x[t - 1] + torch.randn(shape[1:], dtype=torch.float64, device=dev, generator=gen)
    return x


def timed_call(tensors, reps):
    """median ms of one vamp_diag_chains call on device-resident [N, W, D] tensors, HIP events"""
    args = ([t.data_ptr() for t in tensors], True, [t.shape[1] * t.shape[2] for t in tensors], [t.shape[0] for t in tensors],
            [t.shape[1] for t in tensors], [t.shape[2] for t in tensors], 5.0)
    diagnostics._call(0, *args)                       # warm-up: code object load
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = diagnostics._call(0, *args)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), res


def work(shapes):
    fma = sum(W * N * (N + 1) / 2 * D for N, W, D in shapes)
    byt = sum(8 * N * W * D for N, W, D in shapes)
    return fma, byt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libvamp_diag.so")
    ap.add_argument("--label", default="default")
    a = ap.parse_args()
    if a.lib:
        _diag_lib.LIB_PATH = os.path.abspath(a.lib)
    dev = torch.device("cuda", 0)
    out = {"metric": "chain_diagnostics", "label": a.label}
    # q1422-shaped ragged set
    rng = np.random.default_rng(1422)
    Ds = rng.choice([4, 4, 4, 7], size=421)
    host = [ref.ar1(rng, 180, 64, int(D), float(rng.uniform(0.3, 0.95))) for D in Ds]
    shapes = [x.shape for x in host]
    tens = [torch.from_numpy(x).to(dev) for x in host]
    torch.cuda.synchronize()
    med, best, res = timed_call(tens, a.reps)
    t0 = time.perf_counter()
    got = diagnostics.chain_diagnostics(host)
    wall_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = [ref.diagnostics(x) for x in host]
    t_ref = time.perf_counter() - t0
    err = max(float(np.max(np.abs(g.tau / w[0] - 1))) for g, w in zip(got, want))
    fma, byt = work(shapes)
    out["q1422"] = {"groups": len(shapes), "series": int(sum(W * D for _, W, D in shapes)), "N": 180, "W": 64,
                    "event_ms_median": med, "event_ms_min": best, "host_input_wall_ms": wall_host * 1e3,
                    "numpy_restatement_ms": t_ref * 1e3, "fma": fma, "bytes": byt,
                    "frac_fp64_valu": fma / VALU_FP64 / (med * 1e-3), "frac_8TBs": byt / HBM / (med * 1e-3),
                    "max_rel_tau_diff_vs_restatement": err}
    del tens
    torch.cuda.empty_cache()
    if not a.skip_headline:
        N, W, D = 100, 65536, 48
        x = device_ar1((N, W, D), 0.5, 7, dev)
        torch.cuda.synchronize()
        med, best, res = timed_call([x], a.reps)
        sl = 4096
        sub = x[:, :sl].cpu().numpy()
        t0 = time.perf_counter()
        ref.diagnostics(sub)
        t_ref = (time.perf_counter() - t0) * (W / sl)
        fma, byt = work([(N, W, D)])
        out["headline"] = {"N": N, "W": W, "D": D, "event_ms_median": med, "event_ms_min": best,
                           "numpy_restatement_ms_scaled_from_4096_walkers": t_ref * 1e3, "fma": fma, "bytes": byt,
                           "frac_fp64_valu": fma / VALU_FP64 / (med * 1e-3), "frac_8TBs": byt / HBM / (med * 1e-3),
                           "tau_mean": float(np.mean(res[0])), "tau_expected": 3.0}
        del x
        torch.cuda.empty_cache()
        # the same task structure with coalesced staging: 48 groups of [N, W, 1] (lanes read consecutive walkers)
        # instead of one group whose walkers sit D * 8 bytes apart -- isolates the cost of the stride-D gather
        xs = [device_ar1((N, W, 1), 0.5, 100 + d, dev) for d in range(D)]
        torch.cuda.synchronize()
        med1, best1, _ = timed_call(xs, a.reps)
        out["headline_d1_groups"] = {"groups": D, "N": N, "W": W, "D": 1, "event_ms_median": med1, "event_ms_min": best1,
                                     "fma": fma, "bytes": byt}
        del xs
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
