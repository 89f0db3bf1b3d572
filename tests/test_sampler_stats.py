"""CPU tests (-m "not gpu") of tests/sampler_stats.py and, through it, of the stretch move's STATISTICS on the host.

1. The helper checks itself: exact draws against their own CDFs, the quadrature against evidence_ref.quadrature_lnZ and
   the oracle's log_prob, the committed acceptance integrals against a fresh Monte Carlo.
2. Visibility: at the R, W, T of tests/test_gpu_sampler_stats.py the numpy move of the library's semantics is inside every
   bar, and the same move with one rule broken is outside: at D = 3 and D = 4 every broken move misses the KS bar, at every
   D <= 16 the D - 2 exponent and the uniform z miss the acceptance bar.  Run with -s: the table is printed.
3. The GPU file's assertions through oracle/libvamp_cpu.so (the host implementation of the C ABI, bound with _lib.bind as
   tests/test_cpu_boundary.py does) at N = 16 384 walkers.  T is raised where N = 16 384 needs it to meet the cap on se_run
   (prior legs a, b: 800 steps instead of 200; posterior legs: 400 instead of 100); the caps themselves stay.  The legs
   whose host arithmetic costs minutes (d, e, f: 128 .. 600 pixels or 12 .. 17 lines, 800 steps) run on the GPU only.

The numpy move is not run at D = 36 / 68 (leg e): 800 steps of 65 536 walkers take minutes in numpy.
"""
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import vamp_oracle as vo
import evidence_ref as ref
import sampler_stats as ss

N_GPU = 65536
N_HOST = 16384
CPU_SO = os.environ.get("VAMP_CPU_SO") or os.path.join(ROOT, "oracle", "libvamp_cpu.so")


# ---- 1. the helper ---------------------------------------------------------------------------------------------------------
def test_ks_lambda_on_known_cases():
    n = 1000
    grid = (np.arange(n) + 0.5) / n                      # the most uniform sample: D_N = 1 / (2 n)
    assert ss.ks_lambda(grid, lambda v: v) == pytest.approx(0.5 / math.sqrt(n), rel=1e-9)
    assert ss.ks_lambda(grid + 0.1, lambda v: np.clip(v, 0, 1)) == pytest.approx(math.sqrt(n) * (0.1 + 0.5 / n), rel=1e-9)
    assert ss.ks_lambda(np.full(n, 2.0), lambda v: np.clip(v, 0, 1)) == pytest.approx(math.sqrt(n))       # all above the support: D_N = 1


@pytest.mark.parametrize("mode,K,sd", [(vo.MODE_GAUSS3, 1, False), (vo.MODE_VOIGT4, 2, True)])
def test_prior_is_the_oracles_and_its_draws_match_its_cdfs(mode, K, sd):
    x = np.arange(8.0) - 2.0
    target = ss.RegionPrior(mode, K, x, sample_sd=sd)
    region = vo.Region(x=x, flux=np.ones(8), noise=np.ones(8), n_comp=K, mode=mode, sample_sd=sd)
    rng = np.random.default_rng(11)
    X = target.draw(N_GPU, rng)
    lam = [ss.ks_lambda(X[:, d], target.cdf(d)) for d in range(target.D)]
    print("prior draws against their CDFs, mode %d K %d sd %d: lambda" % (mode, K, sd), np.round(lam, 2))
    assert max(lam) < ss.KS_BAR
    pts = np.vstack([X[:40], X[:40] * np.where(np.arange(target.D) == 1, -3.0, 1.0), X[:40] * np.where(np.arange(target.D) == 0, -1.0, 1.0),
                     X[:40] * np.where(np.arange(target.D) == 2, 40.0, 1.0)])
    want = np.array([vo.log_prior(region, t) for t in pts])
    got = target.logp(pts)
    assert np.array_equal(np.isfinite(want), np.isfinite(got)) and not np.isfinite(want).all() and np.isfinite(want).any()
    fin = np.isfinite(want)
    assert np.allclose(got[fin], want[fin], rtol=1e-13, atol=1e-13)
    # the marginal CDFs are the priors': d CDF / dv is exp(log prior) along one axis
    for d in range(target.D):
        lo, hi = (0.0, 12.0) if target.dims[d] is None else target.dims[d]
        v = np.linspace(lo, hi, 2001)
        pdf = v * np.exp(-v) if target.dims[d] is None else np.full(v.size, 1.0 / (hi - lo))
        num = np.gradient(target.cdf(d)(v), v)
        assert np.max(np.abs(num[1:-1] - pdf[1:-1])) < 1e-4
        assert target.cdf(d)(np.array([lo - 1.0]))[0] == 0.0 and target.cdf(d)(np.array([hi + 1e3]))[0] == pytest.approx(1.0, abs=1e-4)


@pytest.mark.parametrize("sample_sd", [False, True], ids=["fixed-noise", "free-sd"])
def test_quadrature_posterior_of_one_gaussian_line(sample_sd):
    for N in (N_GPU, N_HOST):
        g = ss.gauss_line_posterior(sample_sd, N)
        print("quadrature %s for N = %d: n = %d per axis, box %s, eps %.3g (quadrature %.3g + cut mass %.1g) <= %.3g, ln Z %.6f" % (
            "free sd" if sample_sd else "fixed noise", N, g.n, np.round(g.box, 3).tolist(), g.eps, g.eps_quad, ss.MASS_CUT[sample_sd], g.eps_bar, g.lnZ))
        assert g.eps <= g.eps_bar == ss.EPS_FRACTION * ss.KS_BAR / math.sqrt(N)
    g = ss.gauss_line_posterior(sample_sd, N_GPU)
    # the integrand is the oracle's log_prob (up to include_norm, which the sampler's contexts leave off)
    region = vo.Region(x=g.x, flux=g.flux, noise=g.noise, n_comp=1, mode=vo.MODE_GAUSS3, sample_sd=sample_sd)
    rng = np.random.default_rng(12)
    pts = g.draw(60, rng)
    pts[50:, 1] += 20.0                                    # outside the prior
    want = np.array([vo.log_prob(region, t) for t in pts])
    got = g.logp(pts)
    assert np.all(np.isfinite(want[:50])) and np.all(want[50:] == -np.inf) and np.all(got[50:] == -np.inf)
    assert np.allclose(got[:50], want[:50], rtol=1e-12, atol=1e-12)
    if not sample_sd:
        # the normalisation: the midpoint rule of evidence_ref over the whole prior box, which tests/test_evidence.py holds
        # to 8.227 +- 1e-3
        z160 = ref.quadrature_lnZ(g.x, g.flux, g.noise, 160)
        print("ln Z: box quadrature %.9f, evidence_ref.quadrature_lnZ(160) %.9f" % (g.lnZ, z160))
        assert abs(g.lnZ - z160) <= 1e-3
    # exact draws against their own marginal CDFs
    X = g.draw(N_GPU, np.random.default_rng(13))
    lam = [ss.ks_lambda(X[:, d], g.cdf(d)) for d in range(g.D)]
    print("exact draws against the quadrature CDFs: lambda", np.round(lam, 2), "bar %.2f" % (ss.KS_BAR + math.sqrt(N_GPU) * g.eps))
    assert max(lam) < ss.KS_BAR + math.sqrt(N_GPU) * g.eps
    assert np.all(np.isfinite(g.logp(X)))


def test_committed_acceptance_references_against_a_fresh_integral():
    """tests/golden/sampler_stats_acceptance.json (sampler_stats.write_golden) holds every leg's p_acc to se <= 2e-4; a
    fresh Monte Carlo of 2^18 proposals with another seed agrees within 5 joint standard errors"""
    legs = [(name, ss.prior_leg(name)) for name in ss.PRIOR_LEGS] + [("post-fixed", ss.posterior_leg(False, N_GPU)), ("post-sd", ss.posterior_leg(True, N_GPU))]
    for name, (data, target, (p, se)) in legs:
        p2, se2 = ss.acceptance_reference(target.draw, target.logp, target.D, 1 << 18, rng=np.random.default_rng(77))
        print("acceptance integral %-10s D %2d: committed %.5f +- %.5f, fresh %.5f +- %.5f" % (name, target.D, p, se, p2, se2))
        assert se <= ss.SE_REF_CAP
        assert abs(p - p2) <= 5.0 * math.hypot(se, se2)


# ---- 2. visibility ----------------------------------------------------------------------------------------------------------
def _numpy_leg(leg, broken, R, W, seed=5):
    data, target, (p, se) = ss.posterior_leg(leg == "post-sd", R * W) if leg.startswith("post") else ss.prior_leg(leg)
    rng = np.random.default_rng(seed)
    X0 = target.draw(R * W, rng)
    X, lnp, nacc = ss.numpy_stretch(target.logp, X0, R, W, data["T"], rng, broken=broken)
    return ss.leg_figures(X, nacc, R, W, data["T"], target, p, se, corr=not leg.startswith("post"))


VISIBLE = [(leg, b) for leg in ("a", "b") for b in ss.BROKEN] + [(leg, b) for leg in ("f", "d", "c") for b in ("dm2", "zunif")]


@pytest.mark.parametrize("leg,R,W", [("a", 1024, 64), ("a", 16, 4096), ("b", 1024, 64), ("f", 16, 4096), ("d", 1024, 64), ("c", 1024, 64),
                                     ("post-fixed", 1024, 64), ("post-sd", 16, 4096)])
def test_correct_numpy_move_is_inside_every_bar(leg, R, W):
    ss.assert_leg("numpy move, leg %s, %d x %d, correct" % (leg, R, W), _numpy_leg(leg, None, R, W))


@pytest.mark.parametrize("leg,broken", VISIBLE)
def test_broken_numpy_move_is_outside_its_bar(leg, broken):
    fig = _numpy_leg(leg, broken, 1024, 64)
    failed = ss.failed_bars(fig)
    print(ss.format_figures("numpy move, leg %s, 1024 x 64, %s" % (leg, broken), fig), "misses", sorted(failed))
    assert fig["se_ref"] <= ss.SE_REF_CAP
    if leg in ("a", "b"):
        assert "ks" in failed
    if broken in ("dm2", "zunif"):
        assert "acc" in failed and fig["se_run"] <= ss.SE_RUN_CAP


# ---- 3. the GPU file's assertions through the host ABI ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_lib():
    if not os.path.exists(CPU_SO):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
    from vamp_amd import _lib
    return _lib.bind(CPU_SO)


HOST_T = {"a": 800, "b": 800, "c": 800, "post-fixed": 400, "post-sd": 400}      # N = 16 384: see the module's docstring


@pytest.mark.parametrize("leg,R,W", [("a", 256, 64), ("a", 4, 4096), ("b", 256, 64), ("c", 256, 64), ("post-fixed", 256, 64), ("post-sd", 256, 64)])
def test_host_library_leaves_the_target_invariant(cpu_lib, leg, R, W):
    import vamp_amd
    assert R * W == N_HOST
    post = leg.startswith("post")
    data, target, (p, se) = ss.posterior_leg(leg == "post-sd", N_HOST) if post else ss.prior_leg(leg)
    X0 = target.draw(N_HOST, np.random.default_rng(31))
    with vamp_amd.HipContext(lib=cpu_lib) as ctx:
        X, lnp, nacc, _, _ = ss.run_context(ctx, data, X0, R, W, seed=2024, resident=1, T=HOST_T[leg])
        fig = ss.leg_figures(X, nacc, R, W, HOST_T[leg], target, p, se, corr=not post)
        ss.assert_leg("libvamp_cpu.so, leg %s, %d x %d, T %d" % (leg, R, W, HOST_T[leg]), fig)
        ss.assert_state_consistent(ctx, X, lnp, R, W, 1e-9)
