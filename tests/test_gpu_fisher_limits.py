"""GPU tests (-m gpu) of libvamp_fisher.so at its limits, one library call for all of them (tests/fisher_limit_cases.py holds
the case tables and the bars, tests/test_fisher_limits.py the CPU side and the controls):

1. the derivative evaluator entry by entry through ``jac``: every evaluator case of tests/golden/fisher/fisher_limits.npz
   -- y from 0 to 30 across the seam |z|^2 = 64 inside one wavefront, |u| to 1e4, |z| = 7e70 -- at
   |dJ_pd| <= b f |pf_d| S_d + eps (1 + tau) |J_pd|, b = b_core on the identity's sum of absolute terms in the core and
   32 eps on the moduli in the far branch;
2. the information matrix closed on the kernel's own Jacobian: |info_ij - sum_p a_pi a_pj| <= (P + 2) eps sum_p |a_pi a_pj|
   with a = fl(jac fl(1 / sigma)) and the sum in long double, exact symmetry, the free sd's zero row and column;
3. the dealing and factorisation edges (D = 64, 61, 49; triangles of 300, 528, 1035 entries; K = 1, 3, 5; P = 2, 63, 64, 65,
   128) against 40 digits at the bars of tests/fisher_ref.py -- no case is left out by its kappa;
4. cov, sigma and logdet against the exact rational inverse of the kernel's own info down two ladders of merging
   lines: |dS_ij| <= D kappa eps sqrt(S_ii S_jj), |d logdet| <= D kappa eps while D kappa eps < 1/2, status 0 wherever the exact
   smallest pivot of the scaled matrix is at least 16 D eps, one change of status along a ladder.
The worst ratios are printed (profiles/fisher_pointwise.txt holds a run's figures)."""
import os

import numpy as np
import pytest

import fisher_limit_cases as fl
import fisher_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

PATH = os.path.join(GOLDEN, "fisher", "fisher_limits.npz")
EVAL, META = fl.load_eval(PATH)
FULL = ref.load_cases(PATH)
OLD = {c["name"]: c for c in ref.load_cases(os.path.join(GOLDEN, "fisher", "fisher_cases.npz"))}
LADDERS = {m: [dict(zip(("name", "x", "flux", "noise", "theta", "K", "mode"), t), sd=False) for t in fl.ladder(m)] for m in (0, 1)}
ALL = EVAL + FULL + [OLD[n] for n in fl.OLD_CASES] + LADDERS[0] + LADDERS[1]

_cache = {}


def _records():
    """name -> record, from ONE call"""
    if not _cache:
        from vamp_amd import fisher
        recs = fisher.fisher_points([c["x"] for c in ALL], [c["flux"] for c in ALL], [c["noise"] for c in ALL], [c["theta"] for c in ALL],
                                    [c["K"] for c in ALL], [c["mode"] for c in ALL], jac=True)
        _cache.update({c["name"]: r for c, r in zip(ALL, recs)})
        assert len(_cache) == len(ALL)
    return _cache


def test_evaluator_entry_by_entry_through_the_jacobian():
    print(f"E_sc = {META['e_sc']:.3e}  b_core = {META['b_core']:.3e}  far bar = 32 eps")
    worst = {}
    for c in EVAL:
        r = _records()[c["name"]]
        assert r.jac.shape == (c["P"], 4) and r.status in (0, 1)
        worst[c["name"]] = fl.entry_ratios(c, r.jac, META["b_core"])
        print(f"device {c['name']:14s} y={c['y']:.3g} P={c['P']:2d} core {worst[c['name']][0]:.3f} far {worst[c['name']][1]:.3f}")
    for name, (core, far) in worst.items():
        assert core <= 1.0 and far <= 1.0, (name, core, far)


def test_information_closes_on_the_kernels_own_jacobian():
    for c in ALL:
        r = _records()[c["name"]]
        Dl = ref.q_of(c["mode"]) * c["K"]
        sig = np.full(len(c["x"]), c["theta"][-1]) if c["sd"] else c["noise"]
        got = fl.closure_ratio(r.info, r.jac, sig, c["theta"], c["K"], c["mode"], c["sd"])
        print(f"closure {c['name']:24s} D={len(c['theta']):2d} P={len(c['x']):3d} {got:.3f}")
        assert got <= 1.0, (c["name"], got)
        assert np.array_equal(r.info, r.info.T), c["name"]
        if c["sd"]:
            assert np.all(r.info[Dl, :Dl] == 0.0) and np.all(r.info[:Dl, Dl] == 0.0) and np.all(r.jac[:, Dl] == 0.0)
            assert r.info[Dl, Dl] == pytest.approx(2.0 * len(c["x"]) / c["theta"][-1] ** 2, rel=4 * fl.EPS)


def test_dealing_and_pixel_edges_against_40_digits():
    from test_gpu_fisher import _ratios
    for c in FULL:
        r = _records()[c["name"]]
        worst = _ratios(c, r)
        print(f"{c['name']:20s} D={c['D']:2d} P={c['P']:3d} status={r.status} kappa={c['kappa']:.2e} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
        want = {"jac", "grad", "info", "chi2"} | ({"cov", "logdet", "CS-1"} if c["kind"] == "full" else set())
        assert set(worst) == want, (c["name"], sorted(worst))                  # nothing dropped by its kappa
        assert all(v <= 1.0 for v in worst.values()), (c["name"], worst)
        if c["kind"] == "full":
            assert r.status == 0 and np.array_equal(r.cov, r.cov.T) and np.allclose(r.sigma, np.sqrt(np.diag(r.cov)), rtol=1e-15, atol=0)
        else:                                                                  # pixel_P2: rank 4 of 8
            assert r.status == 1 and np.all(np.isnan(r.cov)) and np.isnan(r.logdet) and np.all(np.isfinite(r.info))


def _stage(c, r, sum_rounding=False):
    """the assertions of part 4 on one record; returns (decided, status).  sum_rounding: the cases beside the ladders,
    which were not chosen for this stage, get the rounding of ln det's own sum beside D kappa eps -- 2 eps sum of the
    absolute logarithms -- since a well-conditioned matrix of small entries has |ln det| = 100 and D kappa eps below its ulp"""
    D = len(c["theta"])
    ex = fl.exact_stage(r.info)
    safe = ex is not None and ex["min_pivot"] >= fl.PIVOT_SAFE * D * fl.EPS
    line = f"{c['name']:20s} status={r.status} "
    if ex is not None:
        line += f"kappa={ex['kappa']:.2e} min pivot / (D eps)={ex['min_pivot'] / (D * fl.EPS):.3g} "
    if safe:
        assert r.status == 0, c["name"]
    if r.status == 0:
        assert np.all(np.isfinite(r.cov)) and np.array_equal(r.cov, r.cov.T) and np.all(np.diag(r.cov) > 0) and np.isfinite(r.logdet)
        assert np.allclose(r.sigma, np.sqrt(np.diag(r.cov)), rtol=1e-15, atol=0)
        if ex is not None and D * ex["kappa"] * fl.EPS < 0.5:
            got = fl.stage_ratios(r.cov, r.logdet, ex)
            with np.errstate(all="ignore"):
                inv = fl.stage_ratios(np.linalg.inv(r.info), np.linalg.slogdet(r.info)[1], ex)
            mine = fl.cholesky_copy(r.info)
            line += (f"over kappa eps (bar {D}): kernel cov {got[0]:.3f} logdet {got[1]:.3f}  numpy inv {inv[0]:.3f} {inv[1]:.3f}  "
                     f"numpy copy {fl.stage_ratios(mine[0], mine[1], ex)[0]:.3f}")
            print(line)
            assert got[0] <= D and got[1] <= D + (2.0 * ex["log_terms"] / ex["kappa"] if sum_rounding else 0.0), (c["name"], got)
            return safe, r.status
    else:
        assert r.status == 1 and np.all(np.isnan(r.cov)) and np.all(np.isnan(r.sigma)) and np.isnan(r.logdet)
        assert np.all(np.isfinite(r.grad)) and np.all(np.isfinite(r.info)) and np.all(np.isfinite(r.jac))
    print(line)
    return safe, r.status


@pytest.mark.parametrize("mode", [0, 1], ids=["gauss", "voigt"])
def test_covariance_stage_down_the_ladder(mode):
    out = [_stage(c, _records()[c["name"]]) for c in LADDERS[mode]]
    status = [s for _, s in out]
    assert sum(a != b for a, b in zip(status, status[1:])) <= 1, status
    assert sum(1 for safe, _ in out if not safe) <= 1 and status[0] == 0      # at most one rung in the undecided band
    if mode == 0:
        exact = [fl.exact_stage(_records()[c["name"]].info) for c in LADDERS[0][:-1]]
        assert sum(1 for ex in exact if 1e12 < ex["kappa"] < 0.5 / (6 * fl.EPS)) >= 2                          # compared beyond kappa = 1e12


def test_covariance_stage_on_far_line_and_the_fixture_cases():
    """far_line (kappa = 1.1e15, status 0 in profiles/fisher_limits.txt) and every other case of the call whose D is small
    enough for the rational inverse"""
    _stage(OLD["far_line"], _records()["far_line"])
    took = 0
    for c in EVAL + FULL + [OLD[n] for n in fl.OLD_CASES]:
        if len(c["theta"]) <= 20 and c["name"] != "far_line":
            _stage(c, _records()[c["name"]], sum_rounding=True)
            took += 1
    assert took >= 30
