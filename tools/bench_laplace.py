#!/usr/bin/env python3
"""Cost of Laplace importance sampling (libvamp_laplace.so) on the shape of a q1422 fit, one JSON line:

  421 groups (the region lengths of tests/golden/q1422_spectrum.npz), 1 .. 4 Voigt lines per region, free sd (the form
  every VPregion fit uses), S = 4096 draws per region from N(centre, 1.5^2 Fisher covariance at the centre); the centre
  is the point the data were made from (no fit is run here: what is timed does not depend on where the centre is).

  library   one vamp_laplace_points call from host centres and factors, HIP events around it, after a warm-up call; the
            call includes its allocations, the four kernels and the copy of the results (no per-sample output).  The
            Fisher call that makes the covariances is timed beside it.  These centres are draws from the prior, not
            fits: most of their proposals reach far outside the prior, and a rejected draw skips its pixels.  So the
            call is timed a second time with a proposal of 1 % of every parameter, where every draw walks its pixels.
  numpy     the restatement (tests/laplace_ref.py) on every --ref-every-th region, scaled by S K P, and ``check`` of the
            library's result on those regions
  ladder    with --evidence: one ``evidence.log_evidence`` call (defaults: 16 x 32 walkers, 600 steps) of the same regions
            in the same process, wall clock

--variants also times the wavefront-only build (VAMP_LAPLACE_NARROW=0) that --build-variants made, alternating with the
default build, on the second proposal (another lane width is another order of the chi^2 sum: other last bits).   python tools/bench_laplace.py [--reps 5] [--evidence] [--build-variants | --variants]"""
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
import laplace_ref as ref  # noqa: E402
import posterior_ref as pref  # noqa: E402
from vamp_amd import _laplace_lib, fisher, laplace  # noqa: E402

S, INFLATE, SEED = 4096, 1.5, 1422
VARIANTS = {"wavefront_only": ["VAMP_LAPLACE_NARROW=0"]}


def variant_path(label):
    return os.path.join(ROOT, "vamp_amd", "libvamp_laplace_%s.so" % label)


def workload(seed=1422):
    g = np.load(os.path.join(ROOT, "tests", "golden", "q1422_spectrum.npz"))
    rng = np.random.default_rng(seed)
    xs, fluxes, centres, ks = [], [], [], []
    for s, e in g["region_pixels"]:
        P = int(e - s)
        K = int(rng.choice([1, 1, 2, 3, 4]))
        x = np.arange(P, dtype=np.float64) - 0.5 * (P - 1)
        centre = pref.draw_prior(rng, x, K, 1, 1)[0]
        centre[2::4] += 0.5
        centre[3::4] += 1.0                    # widths of a pixel or more, as a fit's are
        flux = np.exp(-pref.sample_taus(x, centre[None], K, 1)[0].sum(axis=0)) + 0.05 * rng.standard_normal(P)
        xs.append(x); fluxes.append(flux); ks.append(K); centres.append(np.append(centre, 0.05))
    return xs, fluxes, centres, ks


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
    ap.add_argument("--lib", default=None, help="another build of libvamp_laplace.so")
    ap.add_argument("--label", default="default")
    ap.add_argument("--ref-every", type=int, default=40)
    ap.add_argument("--library-only", action="store_true")
    ap.add_argument("--evidence", action="store_true", help="also time one log_evidence call of the same regions")
    ap.add_argument("--variants", action="store_true", help="also time the variant builds (built beforehand by --build-variants)")
    ap.add_argument("--build-variants", action="store_true", help="build the variant libraries and exit (needs no GPU)")
    a = ap.parse_args()
    if a.build_variants:
        import vamp_amd.build as vb
        for label, defines in VARIANTS.items():
            print(vb.build_laplace(out=variant_path(label), defines=defines))
        return
    if a.lib:
        _laplace_lib.LIB_PATH = os.path.abspath(a.lib)
    torch.zeros(1, device="cuda:0")
    xs, fluxes, centres, ks = workload()
    G = len(xs)
    pix = int(sum(x.size for x in xs))
    evals = int(sum(S * x.size * k for x, k in zip(xs, ks)))
    out = {"metric": "laplace_importance_sampling", "label": a.label, "groups": G, "S": S, "inflate": INFLATE, "pixels": pix,
           "lines": int(sum(ks)), "voigt_evaluations": evals}
    fish = lambda: fisher.fisher_points(xs, fluxes, [None] * G, centres, ks, 1)
    out["fisher_call_event_ms"], recs = timed(fish, a.reps)
    factors = [laplace.proposal_factor(r.cov, INFLATE, r.status)[0] for r in recs]
    common = dict(xs=xs, fluxes=fluxes, noises=[None] * G, n_comp=ks, modes=[1] * G, sample_sd=[1] * G, bounds=[None] * G,
                  region_ids=list(range(G)), centres=centres, chols=factors, n_samples=S, seed=SEED)
    call = lambda: laplace._call(0, **common, want=())
    out["host_centres_event_ms"], flat = timed(call, a.reps)
    # the same call with a proposal of 1 % of every parameter: hardly a draw leaves the prior, so every draw walks its pixels
    tight = dict(common, chols=[np.diag(0.01 * np.abs(c) + 1e-3) for c in centres])
    call_tight = lambda: laplace._call(0, **tight, want=())
    out["tight_proposal_event_ms"], flat_tight = timed(call_tight, a.reps)
    out["tight_proposal_draws_rejected_fraction"] = float(flat_tight["n_out"].sum() / (S * G))
    ok = flat["status"] == 0
    with np.errstate(invalid="ignore"):
        out["statuses"] = {str(s): int((flat["status"] == s).sum()) for s in (0, 1, 2)}
        out["khat_at_most_0.7"] = int((flat["khat"][ok] <= 0.7).sum())
        out["median_khat"], out["median_ess"] = float(np.nanmedian(flat["khat"][ok])), float(np.nanmedian(flat["ess"][ok]))
        out["draws_rejected_fraction"] = float(flat["n_out"][ok].sum() / (S * max(1, int(ok.sum()))))
    if a.variants:
        default_lib = _laplace_lib.load()
        out["variants"] = {}
        for label in VARIANTS:
            lib = _laplace_lib.bind(variant_path(label))
            rounds = {"default": [], label: []}
            same = True
            for _ in range(3):
                for name, handle in (("default", default_lib), (label, lib)):
                    _laplace_lib.load = lambda h=handle: h
                    t, res = timed(call_tight, a.reps)
                    rounds[name].append(t["median"])
                    same = same and all(np.array_equal(res[k], flat_tight[k], equal_nan=True) for k in ("n_out", "status"))
            _laplace_lib.load = lambda h=default_lib: h
            out["variants"][label] = {"tight_proposal_event_ms_median_per_round": rounds, "same_counts_and_statuses": bool(same)}
    if not a.library_only:
        sub = [i for i in range(0, G, a.ref_every)]
        pick = lambda v: [v[i] for i in sub]
        part = dict(common, **{k: pick(common[k]) for k in common if isinstance(common[k], list)})
        full = laplace._call(0, **part)
        t0 = time.perf_counter()
        worst = {}
        for j, i in enumerate(sub):
            case = ref.make_case(xs[i], fluxes[i], None, ks[i], 1, centres[i], factors[i], S, SEED, region_id=i)
            want = ref.run(case)
            D = centres[i].size
            got = {k: full[k][j] for k in ("lnZ", "lnZ_se", "lnZ_psis", "khat", "ess", "lnp_centre", "n_out", "status", "theta", "z", "lnp", "lnq", "lw")}
            ov = int(sum(centres[m].size for m in sub[:j]))
            om = int(sum(centres[m].size ** 2 for m in sub[:j]))
            got.update(mean=full["mean"][ov:ov + D], sd=full["sd"][ov:ov + D], cov=full["cov"][om:om + D * D].reshape(D, D))
            assert want["status"] == got["status"], (i, want["status"], got["status"])
            if want["status"] == 0 and np.isfinite(want["lnZ"]):       # (end to end: it carries the evaluator's 1e-9 of ln p)
                worst["lnZ_end_to_end_abs"] = max(worst.get("lnZ_end_to_end_abs", 0.0), abs(float(want["lnZ"]) - float(got["lnZ"])))
            try:
                stages = ref.check(got, case, "region %d" % i)
            except AssertionError as err:       # (a benchmark reports; tests/test_gpu_laplace.py asserts)
                out.setdefault("check_failures", []).append(repr(err.args[0])[:200])
                continue
            for k, v in stages.items():
                worst[k] = max(worst.get(k, 0.0), float(v))
        t_ref = time.perf_counter() - t0
        share = sum(S * xs[i].size * ks[i] for i in sub) / evals
        out["numpy_restatement_and_check_ms"] = {"measured_on_regions": len(sub), "measured": t_ref * 1e3, "scaled_to_all": t_ref * 1e3 / share}
        out["worst_error_over_bar_per_stage"] = worst
    if a.evidence:
        from vamp_amd import evidence
        regs = [{"x": x, "flux": f, "noise": None, "sample_sd": True, "n_comp": k, "mode": 1, "region_id": i}
                for i, (x, f, k) in enumerate(zip(xs, fluxes, ks))]
        t0 = time.perf_counter()
        ev = evidence.log_evidence(regs)
        out["log_evidence_call_wall_ms"] = (time.perf_counter() - t0) * 1e3
        both = ok & (flat["khat"] <= 0.7)
        d = flat["lnZ"][both] - np.array([e.lnZ for e in ev])[both]
        se = np.hypot(flat["lnZ_se"][both], np.array([e.lnZ_se for e in ev])[both])
        out["lnZ_minus_ladder"] = {"regions": int(both.sum()), "median": float(np.median(d)), "median_abs_over_combined_se": float(np.median(np.abs(d) / se))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
