"""CPU tests of the regularised metric (include/vamp_metric.h): the numpy restatement against the
40-digit fixture and against its own ``check``; every planted error failing ``check`` at its stage; the clamps; the measured
bars, the clamp margins and the default sweep count that tests/test_gpu_metric.py and ``vamp_amd.metric`` rely on;
``prior_scales``; the wiring of ``fits_hmc`` / ``fits_laplace`` with the library replaced by the restatement; the default
path calling nothing new; every argument error before any device call; the host-side checks and launch plan under
AddressSanitizer and UBSan as a stand-alone program; the build constants."""
import ctypes as C
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import metric_ref as ref
from conftest import ROOT

G = ref.golden_cases


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------
def test_fixture_is_what_its_script_makes():
    """the inputs of every case are ``family``'s (the eigenvalues take minutes of mpmath and are not recomputed here)"""
    for name, c in G().items():
        spectrum, D = name.rsplit("_D", 1)
        f = ref.family(spectrum, int(D))
        assert np.array_equal(f["mat"], c["mat"]) and np.array_equal(f["scale"], c["scale"]), name
        assert (f["kind"], f["lam_lo"], f["lam_hi"]) == (c["kind"], c["lam_lo"], c["lam_hi"])
        assert c["eig_ref"].shape == (int(D),) and np.all(np.diff(c["eig_ref"]) >= 0)
    assert sorted({len(c["scale"]) for c in G().values()}) == list(ref.DIMS)


def test_schedule_meets_every_pair_once_per_sweep():
    for n in (2, 4, 6, 18, 48, 64, 66):
        seen = set()
        for r in range(n - 1):
            p, q = ref.schedule(n, r)
            assert len(p) == n // 2 and np.all(p < q) and len(set(p) | set(q)) == n          # disjoint
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == n * (n - 1) // 2


@pytest.mark.parametrize("name", ref.case_names())
def test_restatement_against_the_fixture(name):
    c = G()[name]
    D = len(c["scale"])
    res = ref.run(c, ref.MAX_SWEEPS)
    w = ref.check(res, c, ref.golden_bars()[D], ref.MAX_SWEEPS, name)
    assert res["status"] == 0 and all(v <= 1.0 for v in w.values())
    assert w.get("eig", 0.0) <= 1.0 / ref.MEASURED_FACTOR + 1e-12             # the bar is four times the restatement's own worst
    # numpy's own decomposition agrees to the same bar
    B = ref.scaled(c)
    assert np.max(np.abs(np.linalg.eigvalsh(B) - c["eig_ref"])) <= ref.golden_bars()[D]["eig"] * ref.frobenius(B)
    assert (res["n_low"], res["n_high"]) == ref.clamp(c["eig_ref"], c)[1:]
    if name.startswith(("identity", "diagonal")):
        assert res["sweeps_used"] == 1 and res["off"] == 0.0 and np.array_equal(res["eig"], c["eig_ref"])


def test_measured_bars_and_clamp_margins():
    """the bars are pooled by D, at least 8 eps, near the prototype's figures at D = 65; every reference eigenvalue lies
    further than the eig bar from both clamps, so the exact counts hold for all cases"""
    bars = ref.golden_bars()
    for D, b in sorted(bars.items()):
        print(f"D={D:2d} bars in eps: eig {b['eig'] / ref.EPS:.1f} resid {b['resid'] / ref.EPS:.1f} orth {b['orth'] / ref.EPS:.1f}")
        assert all(b[k] >= ref.MIN_BAR_EPS * ref.EPS for k in ("eig", "resid", "orth"))
        assert all(b[k] == max(ref.MEASURED_FACTOR * b["worst"][k], ref.MIN_BAR_EPS * ref.EPS) for k in ("eig", "resid", "orth"))
    assert 100 * ref.EPS < bars[65]["eig"] < 2000 * ref.EPS and 100 * ref.EPS < bars[65]["orth"] < 2000 * ref.EPS
    for name, c in G().items():
        m = ref.clamp_margin(c, bars[len(c["scale"])]["eig"])
        assert m > 2.0, (name, m)


def test_default_sweep_count_is_the_measured_one():
    from vamp_amd import metric
    at65 = [c for c in G().values() if len(c["scale"]) == 65]
    assert len(at65) == len(ref.SPECTRA)
    need = max(ref.run(c, ref.MAX_SWEEPS)["sweeps_used"] for c in at65)
    print("sweeps needed at D = 65:", {c["name"]: ref.run(c, ref.MAX_SWEEPS)["sweeps_used"] for c in at65})
    assert metric.DEFAULT_SWEEPS == ref.default_sweeps(at65) == min(32, need + 4)
    assert all(ref.run(c, ref.MAX_SWEEPS)["sweeps_used"] <= need for c in G().values())


@pytest.mark.parametrize("plant,stage", sorted(ref.PLANTS.items()))
def test_every_planted_error_fails_check_at_its_stage(plant, stage):
    for name in ("cov_zero_D5", "cov_zero_D17", "cov_zero_D65") + (() if plant.startswith("kind 1") else ("wide_D17", "negative_D65", "wide_D4")):
        c = G()[name]
        bars = ref.golden_bars()[len(c["scale"])]
        ref.check(ref.run(c, ref.MAX_SWEEPS), c, bars)
        with pytest.raises(ref.StageError) as e:
            ref.check(ref.run(c, ref.MAX_SWEEPS, plant=plant), c, bars)
        assert e.value.stage == stage, (name, str(e.value))


def test_check_catches_wrong_statuses_and_counts():
    c = G()["negative_D17"]
    bars = ref.golden_bars()[17]
    good = ref.run(c, ref.MAX_SWEEPS)
    for edit, stage in ((dict(n_low=good["n_low"] + 1), "counts"), (dict(status=1), "chol"), (dict(status=3), "status"), (dict(status=2), "status"),
                        (dict(eig=good["eig"][::-1].copy()), "sorted"), (dict(logdet=good["logdet"] * (1 + 1e-12)), "logdet"),
                        (dict(prec=good["prec"] * (1 + 1e-11)), "prec"), (dict(chol=good["chol"].T.copy()), "chol"), (dict(sweeps_used=33), "sweeps")):
        with pytest.raises(ref.StageError) as e:
            ref.check(dict(good, **edit), c, bars)
        assert e.value.stage == stage, (edit.keys(), str(e.value))
    # the statuses of the header
    one = ref.run(c, 1)
    assert one["status"] == 3 and one["sweeps_used"] == 1 and np.isfinite(one["eig"]).all() and np.isnan(one["cov"]).all() and np.isnan(one["logdet"])
    ref.check(one, c, dict(eig=np.inf, resid=np.inf, orth=np.inf), 1)
    bad = dict(c, mat=c["mat"].copy())
    bad["mat"][5, 2] = np.nan
    two = ref.run(bad, ref.MAX_SWEEPS)
    assert two["status"] == 2 and np.isnan(two["eig"]).all() and two["sweeps_used"] == 0
    ref.check(two, bad, bars)
    upper = dict(c, mat=c["mat"].copy())
    upper["mat"][2, 5] = np.nan
    assert ref.run(upper, ref.MAX_SWEEPS)["status"] == 0
    flat = dict(G()["cov_zero_D5"], lam_hi=np.inf)
    st1 = ref.run(flat, ref.MAX_SWEEPS)
    assert st1["status"] == 1 and np.isnan(st1["chol"]).all() and np.isfinite(st1["cov"]).all()
    ref.check(st1, flat, ref.golden_bars()[5])


def test_clamps():
    """lam_lo raises, lam_hi lowers, kind 1 clamps 1 / e; a direction below lam_lo gets exactly the prior's width"""
    s = np.array([2.0, 0.5, 4.0])
    info = np.diag([1e-6, 9.0, 1e15]) / np.outer(s, s)
    r = ref.run(ref.make_case(info, s, 0, 1.0, 2.0 ** 40), 8)
    assert (r["n_low"], r["n_high"], r["status"]) == (1, 1, 0)
    assert np.allclose(np.diag(r["cov"]), [s[0] ** 2, s[1] ** 2 / 9.0, s[2] ** 2 * 2.0 ** -40], rtol=1e-14)
    assert r["logdet"] == pytest.approx(math.log(9.0) + 40 * math.log(2.0) - 2 * np.sum(np.log(s)))
    assert np.allclose(r["prec"] @ r["cov"], np.eye(3), atol=1e-12) and np.allclose(r["chol"] @ r["chol"].T, r["cov"], rtol=1e-14)
    cov = np.diag([4.0, 1.0 / 9.0, 0.0]) * np.outer(s, s)
    k = ref.run(ref.make_case(cov, s, 1, 1.0, 2.0 ** 40), 8)
    assert (k["n_low"], k["n_high"]) == (1, 1) and np.allclose(np.sort(np.diag(k["cov"]) / s ** 2), [2.0 ** -40, 1.0 / 9.0, 1.0], rtol=1e-14)
    wide = ref.run(ref.make_case(cov, s, 1, 1.0, np.inf), 8)
    assert wide["n_high"] == 0 and wide["status"] == 1


# ---- 2. duplicate lines: where the Fisher factor fails ----------------------------------------------------------------------
@pytest.mark.parametrize("n_lines", [2, 3])
def test_duplicate_lines_have_no_fisher_factor_and_three_repaired_directions(n_lines):
    import fisher_ref
    from vamp_amd import metric
    x, flux, noise, theta = ref.duplicate_lines_case(n_lines)
    f, J = fisher_ref.jacobian(x, theta, n_lines, 1)
    info = fisher_ref.from_jacobian(J, f, flux, noise, theta, n_lines, 1)["info"]
    assert ref.cholesky(info) is None                                # include/vamp_fisher.h's rule: status 1
    case = ref.make_case(info, metric.prior_scales(x, n_lines, 1, False))
    res = ref.run(case, metric.DEFAULT_SWEEPS)
    print("eig in prior units:", res["eig"])
    assert res["status"] == 0 and res["n_low"] >= 3 and res["n_high"] == 0
    ref.check(res, case, ref.measured_bars([case])[theta.size])


# ---- 3. the Python module -----------------------------------------------------------------------------------------------------
def test_prior_scales():
    from vamp_amd import hmc, metric
    x = np.arange(24.0)
    lo, hi, wmax = hmc.derived_bounds(x, 1)
    r12 = math.sqrt(12.0)
    s = metric.prior_scales(x, 2, 1, True)
    assert np.allclose(s, [math.sqrt(2.0), 23.0 / r12, wmax / r12, wmax / r12] * 2 + [1.0 / r12], rtol=0, atol=0)
    g = metric.prior_scales(x[::-1], 3, 0, False)
    assert g.shape == (9,) and np.allclose(g[:3], [math.sqrt(2.0), 23.0 / r12, 11.5 / r12])
    # they are the priors' standard deviations: A e^-A has variance 2, a uniform on a range w has w^2 / 12
    a = np.linspace(0.0, 60.0, 600001)
    pdf = a * np.exp(-a)
    trapezoid = lambda y: float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(a)))
    mean = trapezoid(a * pdf)
    assert mean == pytest.approx(2.0, rel=1e-6) and trapezoid((a - mean) ** 2 * pdf) == pytest.approx(2.0, rel=1e-6)
    with pytest.raises(ValueError, match="mode 2"):
        metric.prior_scales(x, 1, 2, False)


def _fits(n=2, chain=False):
    x = np.arange(24.0)
    out = []
    for i in range(n):
        f = types.SimpleNamespace(_x=x, _flux=np.ones(24), noise=np.full(24, 0.1), _sample_sd=False, _n=1, _mode=0, _scale=np.array([1.0, 2.0, 2.0]),
                                  _shift=np.array([0.0, 1000.0, 0.0]), _names=["A", "c", "s"], _theta_dev=np.array([1.0, 11.0, 2.0]), _chain_dev=None)
        f._set_laplace = lambda rec, args, f=f: setattr(f, "_laplace", (args, rec))
        if chain:
            f._chain_dev = f._theta_dev + 0.1 * np.random.default_rng(i).standard_normal((50, 8, 3)) * np.array([1.0, 1.0, 0.0])
        out.append(f)
    return out


def test_fits_metric_converts_the_information_and_takes_the_chain(monkeypatch):
    from vamp_amd import fisher, metric
    fits = _fits(2, chain=True)
    info_dev = np.array([[400.0, 3.0, 0.0], [3.0, 25.0, 0.0], [0.0, 0.0, 0.0]])            # singular: sigma is not constrained
    recs = [types.SimpleNamespace(info=info_dev / np.outer(f._scale, f._scale), status=1) for f in fits]
    monkeypatch.setattr(fisher, "fits_fisher", lambda fs, device=0: recs)
    calls = []
    monkeypatch.setattr(metric, "regularise", ref.fake_regularise(calls))
    out = metric.fits_metric(fits)
    assert len(calls) == 1 and calls[0]["kind"] == "info" and np.allclose(calls[0]["mats"][0], info_dev, rtol=1e-15)
    scale = metric.prior_scales(fits[0]._x, 1, 0, False)
    assert np.array_equal(calls[0]["scales"][0], scale)
    assert out[0].status == 0 and out[0].n_low >= 1 and out[0].cov[2, 2] == pytest.approx(scale[2] ** 2)        # the prior's width
    by_chain = metric.fits_metric(fits, source="chain")
    assert calls[1]["kind"] == "cov" and np.allclose(calls[1]["mats"][1], np.cov(fits[1]._chain_dev.reshape(-1, 3), rowvar=False))
    assert by_chain[0].status == 0 and by_chain[0].n_high == 1                       # the chain never moved sigma
    with pytest.raises(ValueError, match="source"):
        metric.fits_metric(fits, source="hessian")
    with pytest.raises(ValueError, match="chain"):
        metric.fits_metric(_fits(1), source="chain")
    assert metric.fits_metric([]) == []


def test_fits_hmc_and_fits_laplace_take_the_regularised_metric(monkeypatch):
    """where the Fisher path reports status 1, metric="regularised" hands the library a factor; status 1 is then a metric
    status other than 0; the records say what was repaired"""
    from test_hmc import FakeHmc
    from vamp_amd import fisher, hmc, laplace, metric
    fits = _fits(2)
    info_dev = np.array([[400.0, 3.0, 0.0], [3.0, 25.0, 0.0], [0.0, 0.0, 0.0]])
    infos = [info_dev, np.where(np.eye(3) > 0, np.nan, 0.0)]                          # the second fit: a bad point
    frecs = [types.SimpleNamespace(info=m / np.outer(f._scale, f._scale), cov=np.full((3, 3), np.nan), status=s) for f, m, s in zip(fits, infos, (1, 2))]
    monkeypatch.setattr(fisher, "fits_fisher", lambda fs, device=0: frecs)
    calls = []
    monkeypatch.setattr(metric, "regularise", ref.fake_regularise(calls))
    fake = FakeHmc()
    monkeypatch.setattr(hmc, "_call", fake)
    plain = hmc.fits_hmc(fits, n_chains=4, n_steps=20, n_burn=5)
    assert [r.status for r in plain] == [1, 1] and plain[0].chain is None and plain[0].metric == "fisher" and plain[0].n_low is None and not calls
    out = hmc.fits_hmc(fits, n_chains=4, n_steps=20, n_burn=5, metric="regularised")
    assert len(calls) == 1 and [r.status for r in out] == [0, 1] and out[0].chain.shape == (15, 4, 3) and out[1].chain is None
    assert out[0].metric == "regularised" and out[0].n_low >= 1 and out[0].n_high == 0 and (out[1].n_low, out[1].n_high) == (0, 0)
    want = ref.run(ref.make_case(info_dev, metric.prior_scales(fits[0]._x, 1, 0, False)), metric.DEFAULT_SWEEPS)
    assert np.array_equal(fake.seen[-1]["chols"][0], want["chol"]) and np.isnan(fake.seen[-1]["chols"][1]).all()
    with pytest.raises(ValueError, match="metric"):
        hmc.fits_hmc(fits, metric="hessian")
    # Laplace: the proposal's covariance
    seen = []

    def fake_points(xs, fluxes, noises, centres, covs, n_comp, mode, statuses=None, **kw):
        seen.append(dict(covs=covs, statuses=statuses))
        return [laplace.LaplaceRecord(mean=np.array(c), sd=np.ones(3), cov=np.array(v), status=int(st != 0)) for c, v, st in zip(centres, covs, statuses)]
    monkeypatch.setattr(laplace, "laplace_points", fake_points)
    lap = laplace.fits_laplace(fits, n_samples=64, metric="regularised")
    assert seen[-1]["statuses"] == [0, 2] and np.array_equal(seen[-1]["covs"][0], want["cov"])
    assert [r.status for r in lap] == [0, 1] and lap[0].metric == "regularised" and lap[0].n_low == out[0].n_low
    assert fits[0]._laplace[0] == (64, 1.5, laplace.DEFAULT_SEED, "regularised")
    laplace.fits_laplace(fits, n_samples=64)
    assert seen[-1]["statuses"] == [1, 2] and fits[0]._laplace[0] == (64, 1.5, laplace.DEFAULT_SEED)          # the key of before
    with pytest.raises(ValueError, match="metric"):
        laplace.fits_laplace(fits, metric="hessian")


def test_default_path_calls_nothing_new(monkeypatch):
    """without the keyword neither the metric module nor its library is touched"""
    from test_hmc import FakeHmc
    from vamp_amd import _metric_lib, fisher, hmc, laplace, metric
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the default path reached the metric"))
    for name in ("regularise", "fits_metric", "prior_scales", "_call"):
        monkeypatch.setattr(metric, name, boom)
    monkeypatch.setattr(_metric_lib, "load", boom)
    fits = _fits(2)
    cov = np.diag([0.01, 0.04, 0.04])
    frecs = [types.SimpleNamespace(cov=cov * np.outer(f._scale, f._scale), status=0) for f in fits]
    monkeypatch.setattr(fisher, "fits_fisher", lambda fs, device=0: frecs)
    fake = FakeHmc()
    monkeypatch.setattr(hmc, "_call", fake)
    out = hmc.fits_hmc(fits, n_chains=4, n_steps=20, n_burn=5)
    assert [r.status for r in out] == [0, 0] and np.allclose(np.tril(fake.seen[0]["chols"][0]), np.diag([0.1, 0.2, 0.2]))
    monkeypatch.setattr(laplace, "laplace_points", lambda *a, statuses=None, **k: [laplace.LaplaceRecord(mean=np.ones(3), sd=np.ones(3), cov=np.eye(3), status=0)
                                                                                  for _ in statuses])
    assert [r.metric for r in laplace.fits_laplace(fits, n_samples=64)] == ["fisher", "fisher"]
    # the command line: no --metric, no keyword
    from vamp_amd import do_vamp
    src = open(do_vamp.__file__).read()
    assert 'spec.hmc() if getattr(args, "metric", "fisher") == "fisher"' in src


# ---- 4. the library boundary ----------------------------------------------------------------------------------------------------
def _header_src():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vamp_metric.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def metric_lib():
    import vamp_amd.build as vb
    return vb.build_metric(verbose=False)


def test_metric_library_builds_and_exports_the_header(metric_lib):
    names = sorted(set(re.findall(r"\b(vamp_metric_[a-z0-9_]+)\s*\(", _header_src())))
    assert names == ["vamp_metric_factor", "vamp_metric_last_error", "vamp_metric_plan", "vamp_metric_version"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", metric_lib], text=True)
    assert sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out))) == names
    from vamp_amd import _metric_lib
    assert sorted(_metric_lib.SIGNATURES) == names
    assert len(_metric_lib.SIGNATURES["vamp_metric_factor"][1]) == len(re.search(r"vamp_metric_factor\s*\(([^)]*)\)", _header_src()).group(1).split(","))


def test_build_makes_eleven_libraries_and_the_constants_agree():
    import vamp_amd.build as vb
    from vamp_amd import metric
    assert vb.build(verbose=False).endswith("libvamp_hip.so") and "eleven" in vb.build.__doc__
    for stem in ("hip", "diag", "post", "evid", "pred", "loo", "relabel", "fisher", "laplace", "hmc", "metric"):
        assert os.path.exists(os.path.join(ROOT, "vamp_amd", f"libvamp_{stem}.so")), stem
    assert vb.METRIC_FLAGS is vb.SIDE_FLAGS and vb.METRIC_OUT.endswith("libvamp_metric.so")
    csrc = lambda f: os.path.join(vb.HERE, "csrc", f)
    assert set(vb.METRIC_DEPS) == {vb.METRIC_SRC, os.path.join(vb.HERE, "..", "include", "vamp_metric.h")} | \
        {csrc(f) for f in ("side_call.hpp", "lane_group.hpp", "voigt_math.hpp", "metric_host.hpp")}
    assert set(re.findall(r'#include "([^"]+)"', open(vb.METRIC_SRC).read())) == {"../../include/vamp_metric.h", "lane_group.hpp", "metric_host.hpp",
                                                                                "side_call.hpp"}
    host = open(csrc("metric_host.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", host).lower()                                   # plain C++
    hdr = open(os.path.join(ROOT, "include", "vamp_metric.h")).read()
    assert re.search(r"#define VAMP_METRIC_MAX_DIM %d\b" % metric.MAX_DIM, hdr) and re.search(r"kMaxDim = %d;" % metric.MAX_DIM, host)
    assert re.search(r"#define VAMP_METRIC_MAX_SWEEPS %d\b" % metric.MAX_SWEEPS, hdr) and re.search(r"kMaxSweeps = %d;" % metric.MAX_SWEEPS, host)
    assert "#define VAMP_METRIC_MAX_MATRIX_DOUBLES (1LL << 27)" in hdr and "kMaxMatrixDoubles = 1LL << 27;" in host
    assert metric.MAX_DIM == ref.MAX_DIM == 65 and metric.MAX_SWEEPS == ref.MAX_SWEEPS == 32 and metric.KINDS == {"info": 0, "cov": 1}
    # no workgroup barrier in the kernel: the wavefronts of a workgroup finish in different sweeps
    kernel = re.sub(r"//.*", "", open(vb.METRIC_SRC).read())
    assert "__syncthreads" not in kernel and "lds_fence()" in kernel


def test_launch_plan(metric_lib):
    """matrices per workgroup fall until the LDS fits; the row stride is odd; one matrix of D = 65 needs the raised limit"""
    from vamp_amd import metric
    seen = {}
    for D in range(1, 66):
        per_wg, lds = metric.plan(D)
        n = D + (D & 1)
        slot = 8 * (2 * n * (n + 1) + 7 * n)
        assert lds == per_wg * slot and lds <= 159 * 1024 and (per_wg == 4 or (per_wg + 1) * slot > 159 * 1024)
        seen[D] = per_wg
    assert seen[1] == seen[48] == 4 and seen[65] == 2 and metric.plan(65)[1] // 2 > 64 * 1024 and metric.plan(48)[1] // 4 < 64 * 1024
    from vamp_amd import _metric_lib
    with pytest.raises(_metric_lib.MetricError, match="max_dim = 66"):
        metric.plan(66)


def test_arguments_are_checked_before_any_device_call(metric_lib):
    """none of these reaches hipGetDeviceCount: on a machine without a GPU that call is what fails"""
    from vamp_amd import _metric_lib, metric
    lib = _metric_lib.load()
    assert lib.vamp_metric_version() == 1
    m, s = np.eye(3), np.ones(3)
    base = dict(mats=[m], ld=[3], dims=[3], n_mats=[1], scales=[s], kinds=[0], lam_lo=[1.0], lam_hi=[2.0 ** 40], n_sweeps=8)

    def call(**kw):
        with pytest.raises(_metric_lib.MetricError) as e:
            metric._call(0, **dict(base, **kw))
        assert "hip" not in str(e.value).lower()
        return str(e.value)

    assert "n_sweeps = 0 is outside 1 .. 32" in call(n_sweeps=0)
    assert "n_sweeps = 33 is outside" in call(n_sweeps=33)
    assert "dim = 0 is outside 1 .. 65" in call(dims=[0])
    assert "dim = 66 is outside" in call(dims=[66])
    assert "n_mat must be at least 1" in call(n_mats=[0])
    assert "ld = 2 is below the 3 entries" in call(ld=[2])
    assert "kind must be 0" in call(kinds=[2])
    assert "scale must be positive and finite (entry 1)" in call(scales=[np.array([1.0, 0.0, 1.0])])
    assert "scale must be positive and finite (entry 2)" in call(scales=[np.array([1.0, 1.0, np.inf])])
    assert "lam_lo must be positive" in call(lam_lo=[0.0])
    assert "lam_lo must be positive" in call(lam_lo=[np.inf], lam_hi=[np.inf])
    assert "lam_hi must be at least lam_lo" in call(lam_lo=[2.0], lam_hi=[1.0])
    assert "lam_hi must be at least lam_lo" in call(lam_hi=[np.nan])
    assert "matrix entries" in call(mats=[np.zeros((1, 65, 65))], dims=[65], ld=[65], n_mats=[1 << 15], scales=[np.ones(65)], skip=("vec", "cov", "prec", "chol"))
    assert "to copy from host memory" in call(ld=[1 << 26], n_mats=[8])
    assert "ld is beyond" in call(ld=[(1 << 27) + 1])
    two = dict(base, mats=[m, m], ld=[3, 3], dims=[3, 3], n_mats=[1, 1], kinds=[0, 0], lam_lo=[1.0, 1.0], lam_hi=[2.0, 2.0])
    assert "group 1: scale must be" in call(**dict(two, scales=[s, -s]))
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    vp = (C.c_void_p * 1)(m.ctypes.data)
    sp = (C.c_void_p * 1)(s.ctypes.data)
    i32 = lambda v: np.array([v], dtype=np.int32).ctypes.data_as(ip)
    f64 = lambda v: np.array([v], dtype=np.float64).ctypes.data_as(dp)
    ld = np.array([3], dtype=np.int64).ctypes.data_as(lp)
    raw = lambda groups=1, is_dev=0, out_dev=0, mat=vp: lib.vamp_metric_factor(0, None, groups, mat, is_dev, ld, i32(3), i32(1), sp, i32(0), f64(1.0),
                                                                            f64(2.0), 8, out_dev, *([None] * 11))
    assert raw(groups=0) == -1 and b"n_groups" in lib.vamp_metric_last_error()
    assert raw(is_dev=2) == -1 and b"is_device" in lib.vamp_metric_last_error()
    assert raw(out_dev=2) == -1 and b"out_is_device" in lib.vamp_metric_last_error()
    assert raw(mat=None) == -1 and b"NULL argument" in lib.vamp_metric_last_error()
    assert raw(mat=(C.c_void_p * 1)(None)) == -1 and b"NULL matrix or scale" in lib.vamp_metric_last_error()
    # what Python refuses itself
    for kw, match in ((dict(mats=np.eye(3), scales=np.ones(4)), "do not belong"), (dict(mats=np.ones((2, 3)), scales=np.ones(3)), "neither"),
                      (dict(mats=np.eye(3), scales=np.ones(3), kind="hessian"), "kind"), (dict(mats=np.eye(3), scales=-np.ones(3)), "positive and finite"),
                      (dict(mats=np.eye(3), scales=np.ones(3), lam_lo=0.0), "lam_lo"), (dict(mats=np.eye(3), scales=np.ones(3), lam_lo=2.0, lam_hi=1.0), "lam_lo"),
                      (dict(mats=np.eye(3), scales=np.ones(3), n_sweeps=33), "n_sweeps"), (dict(mats=np.eye(3), scales=np.ones(3), want=("jac",)), "unknown outputs"),
                      (dict(mats=[np.eye(3)], scales=[np.ones(3)] * 2), "one set of scales"), (dict(mats=np.eye(66), scales=np.ones(66)), "D = 66")):
        with pytest.raises(ValueError, match=match):
            metric.regularise(**kw)
    assert metric.regularise([], []) == []


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mt") / "metric_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "metric_host.cpp")])
    return exe


def test_host_checks_and_plan_under_sanitizers(host_exe):
    """tests/host/metric_host.cpp: the argument checks, the layout and the plan of metric_host.hpp, stand-alone, under
    AddressSanitizer and UBSan; its plan table is the library's"""
    rc = subprocess.run([host_exe], capture_output=True, text=True, timeout=120)
    assert rc.returncode == 0, rc.stdout[-2000:] + rc.stderr[-4000:]
    lines = [ln.split() for ln in rc.stdout.splitlines() if ln.startswith("plan ")]
    assert len(lines) == 65
    for _, D, waves, lds in lines:
        n = int(D) + (int(D) & 1)
        assert int(lds) == int(waves) * 8 * (2 * n * (n + 1) + 7 * n)
    assert "checks ok" in rc.stdout
