#!/usr/bin/env python3
"""Cost of preconditioned HMC (libvamp_hmc.so) on the shape of a q1422 fit, one JSON line:

  421 groups (the region lengths of tests/golden/q1422_spectrum.npz), 1 .. 4 Voigt lines per region, free sd (the form
  every VPregion fit uses), 16 chains per region, L = 8 leapfrog steps per move; the chains start on the point the data
  were made from, in a metric of 1 % of every parameter at a step size small enough that hardly a trajectory meets a
  wall (no fit is run here: what is timed is L gradient evaluations per move, wherever the chain is).

  library   one vamp_hmc_chains call from host starts and factors, HIP events around it, after a warm-up call; the call
            includes its allocations, the resident kernel and the copy of the kept states.  Reported: ms per call and
            gradient evaluations per second (moves x L x chains, less what the walls cut short).
  variants  with --variants: the build with the butterfly reduction of the gradient (VAMP_HMC_TREE=1, made by
            --build-variants) alternating with the default build (lane d folds row d of the tile in pixel order); another
            order of summation is other last bits, so the two are compared on their counts, not bit for bit.
  numpy     the restatement (tests/hmc_ref.py) on every --ref-every-th region, scaled by moves x chains x K x P, and
            ``check`` of the library's result on those regions

--convergence measures, and gates nothing: on the quadrature case (one Gaussian line, 24 pixels) and on one four-line
Voigt blend, ``fits_hmc`` at its default budget -- worst split-R-hat and least n_eff over the parameters -- beside
``mcmc_fit`` (the stretch move) at the product's default budget (3000 iterations, burn 300, thin 15).

    python tools/bench_hmc.py [--reps 5] [--steps 50] [--build-variants | --variants] [--convergence]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHAINS, LEAP, SEED, EPS = 16, 8, 1422, 0.3
VARIANTS = {"tree": ["VAMP_HMC_TREE=1"]}


def variant_path(label):
    return os.path.join(ROOT, "vamp_amd", "libvamp_hmc_%s.so" % label)


def workload(seed=1422):
    import posterior_ref as pref
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
    import torch
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


def convergence():
    """worst split-R-hat and least n_eff of HMC at its default budget and of the stretch move at the product's, on the
    quadrature case and on a four-line Voigt blend"""
    import evidence_ref
    from oracle import vamp_oracle as vo
    from vamp_amd.vpfits import VPfit
    out = {}
    x, flux, noise = evidence_ref.gauss_line_data(24, [(1.2, 11.3, 2.5)], 0.1, 3)
    xb = np.arange(64.0)
    truth = np.array([[0.9, 24.0, 1.0, 4.0], [1.4, 29.0, 0.8, 3.5], [0.7, 35.0, 1.2, 4.5], [1.1, 40.0, 0.6, 3.0]]).ravel()
    R = vo.Region(x=xb, flux=np.ones(64), noise=np.ones(64), n_comp=4, mode=1)
    fb = vo.model_flux(R, truth) + 0.03 * np.random.default_rng(9).standard_normal(64)
    for name, (xx, ff, nn, K, voigt) in {"quadrature_one_gauss_line": (x, flux, noise, 1, False),
                                         "four_line_voigt_blend": (xb, fb, np.full(64, 0.03), 4, True)}.items():
        fit = VPfit(noise=nn, seed=5)
        fit.initialise_model(1.0e3 + 2.0 * xx, ff, K, voigt=voigt)
        fit.map_estimate()
        t0 = time.perf_counter()
        rec = fit.hmc()
        t_hmc = time.perf_counter() - t0
        d = rec.diagnostics() if rec.status == 0 else None
        row = {"hmc": {"status": int(rec.status), "seconds": t_hmc, "eps": rec.eps, "n_steps": rec.n_steps, "n_leap": rec.n_leap,
                       "accept_rate": None if rec.status else float(np.nanmean(rec.accept_rate)),
                       "n_wall": None if rec.status else int(np.sum(rec.n_wall)),
                       "max_r_hat": None if d is None else float(np.nanmax(d.r_hat)), "min_n_eff": None if d is None else float(np.nanmin(d.n_eff)),
                       "tau_reliable": None if d is None else bool(np.all(d.reliable))}}
        t0 = time.perf_counter()
        fit.mcmc_fit(iterations=3000, burnin=300, thinning=15)
        t_mc = time.perf_counter() - t0
        dm = fit.mcmc.diagnostics()
        row["stretch_move"] = {"seconds": t_mc, "iterations": 3000, "burn": 300, "thin": 15, "walkers": int(fit._chain_dev.shape[1]),
                               "max_r_hat": float(np.nanmax([v["r_hat"] for v in dm.values()])),
                               "min_n_eff": float(np.nanmin([v["n_eff"] for v in dm.values()])),
                               "tau_reliable": bool(all(v["reliable"] for v in dm.values()))}
        out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="moves per call")
    ap.add_argument("--lib", default=None, help="another build of libvamp_hmc.so")
    ap.add_argument("--label", default="default")
    ap.add_argument("--ref-every", type=int, default=10)
    ap.add_argument("--ref-steps", type=int, default=3, help="moves the restatement makes per chain")
    ap.add_argument("--library-only", action="store_true")
    ap.add_argument("--variants", action="store_true", help="also time the variant builds (built beforehand by --build-variants)")
    ap.add_argument("--build-variants", action="store_true", help="build the variant libraries and exit (needs no GPU)")
    ap.add_argument("--convergence", action="store_true", help="also measure R-hat and n_eff of HMC and of the stretch move on two cases")
    a = ap.parse_args()
    if a.build_variants:
        import vamp_amd.build as vb
        for label, defines in VARIANTS.items():
            print(vb.build_hmc(out=variant_path(label), defines=defines))
        return
    import torch
    import hmc_ref as ref
    from vamp_amd import _hmc_lib, hmc
    if a.lib:
        _hmc_lib.LIB_PATH = os.path.abspath(a.lib)
    torch.zeros(1, device="cuda:0")
    xs, fluxes, centres, ks = workload()
    G = len(xs)
    chols = [np.diag(0.01 * np.abs(c) + 1e-3) for c in centres]
    starts = [np.tile(c, (CHAINS, 1)) for c in centres]
    common = dict(xs=xs, fluxes=fluxes, noises=[None] * G, n_comp=ks, modes=[1] * G, sample_sd=[1] * G, bounds=[None] * G,
                  region_ids=list(range(G)), n_chains=[CHAINS] * G, chain_id0=[0] * G, starts=starts, chols=chols, eps=[EPS] * G,
                  jitter=[0.2] * G, n_leap=LEAP, n_steps=a.steps, n_burn=0, thin=1, seed=SEED)
    call = lambda: hmc._call(0, **common, want=())
    out = {"metric": "hmc_chains", "label": a.label, "groups": G, "chains_per_group": CHAINS, "n_leap": LEAP, "n_steps": a.steps,
           "pixels": int(sum(x.size for x in xs)), "lines": int(sum(ks))}
    out["call_event_ms"], flat = timed(call, a.reps)
    moves = G * CHAINS * a.steps
    out["chain_status"] = {str(s): int((flat["chain_status"] == s).sum()) for s in (0, 1, 2)}
    out["accept_rate"], out["wall_fraction"] = float(flat["n_accept"].sum() / moves), float(flat["n_wall"].sum() / moves)
    out["gradient_evaluations_per_call_upper"] = moves * LEAP
    out["gradient_evaluations_per_second"] = moves * LEAP / (out["call_event_ms"]["median"] * 1e-3)
    if a.variants:
        default_lib = _hmc_lib.load()
        out["variants"] = {}
        for label in VARIANTS:
            lib = _hmc_lib.bind(variant_path(label))
            rounds = {"default": [], label: []}
            counts = {}
            for _ in range(3):
                for name, handle in (("default", default_lib), (label, lib)):
                    _hmc_lib.load = lambda h=handle: h
                    t, res = timed(call, a.reps)
                    rounds[name].append(t["median"])
                    counts[name] = (int(res["n_accept"].sum()), int(res["n_wall"].sum()))
            _hmc_lib.load = lambda h=default_lib: h
            out["variants"][label] = {"call_event_ms_median_per_round": rounds, "accepted_and_walls": counts}
    if not a.library_only:
        sub = list(range(0, G, a.ref_every))
        pick = lambda v: [v[i] for i in sub]
        part = dict(common, **{k: pick(common[k]) for k in common if isinstance(common[k], list)}, n_steps=a.ref_steps)
        full = hmc._call(0, **part)
        t0 = time.perf_counter()
        worst = {}
        for j, i in enumerate(sub):
            case = ref.make_case(xs[i], fluxes[i], None, ks[i], 1, starts[i], chols[i], EPS, LEAP, a.ref_steps, SEED, jitter=0.2, region_id=i)
            t1 = time.perf_counter()
            ref.run(case)
            out["numpy_run_seconds"] = out.get("numpy_run_seconds", 0.0) + time.perf_counter() - t1
            o = j * CHAINS
            got = {k: full[k][o:o + CHAINS] for k in ("n_accept", "n_wall", "chain_status", "dH_mean", "dH_max")}
            got.update({k: full[k][j] for k in ("chain", "last", "lnp", "mom", "prop", "prop_mom", "dH", "acc")}, status=int(full["status"][j]))
            try:
                stages = ref.check(got, case, "region %d" % i, bars=ref.measured_bars(case))
            except AssertionError as err:       # (a benchmark reports; tests/test_gpu_hmc.py asserts)
                out.setdefault("check_failures", []).append(repr(err.args[0])[:200])
                continue
            for k, v in stages.items():
                worst[k] = max(worst.get(k, 0.0), float(v))
        work = lambda idx, steps: sum(steps * CHAINS * xs[i].size * ks[i] for i in idx)
        share = work(sub, a.ref_steps) / work(range(G), a.steps)
        out["numpy_restatement_ms"] = {"measured_on_regions": len(sub), "moves_per_chain": a.ref_steps, "measured": out.pop("numpy_run_seconds") * 1e3}
        out["numpy_restatement_ms"]["scaled_to_the_call"] = out["numpy_restatement_ms"]["measured"] / share
        out["check_seconds"] = time.perf_counter() - t0
        out["worst_error_over_bar_per_stage"] = worst
    if a.convergence:
        out["convergence"] = convergence()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
