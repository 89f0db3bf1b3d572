"""CPU tests of the pointwise predictive density and WAIC: the numpy restatement (tests/predictive_ref.py) against a
brute-force loop in extended precision, the libvamp_pred.so boundary (build, exports, ctypes table, argument checks
before any device call), the Python wiring (mcmc.waic, fits_predictive's time step, VPspectrum.predictive, do_vamp
--predictive, the WAIC ladder of VPregion) with the library call replaced by the restatement, and the planted errors the
GPU comparison's bars must catch."""
import ctypes as C
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

import posterior_ref as pref
import predictive_ref as ref
from conftest import ROOT, load_golden
from oracle import vamp_oracle as vo


def _golden(name="H1215_r0_K4_m1_sd0"):
    g = load_golden("lnprob_cases.npz")
    fin = np.isfinite(g[name + "_lnprob"])
    return g[name + "_x"], g[name + "_flux"], g[name + "_noise"], g[name + "_theta"][fin][0]


def _ball_case(seed, S, sample_sd, name="H1215_r0_K4_m1_sd0", K=4, mode=1):
    """a chain like a converged one: a 1 % ball around a fitted point (with free sd: around sd = the data's noise level)"""
    x, flux, noise, th = _golden(name)
    rng = np.random.default_rng(seed)
    centre = np.append(th[:(4 if mode == 1 else 3) * K], float(np.median(noise))) if sample_sd else th
    return x, flux, (None if sample_sd else noise), pref.ball(rng, centre, S)


# ---- the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_sd", [False, True])
def test_restatement_against_a_brute_force_loop(sample_sd):
    x, flux, noise, theta = _ball_case(41, 12 * 5, sample_sd)
    theta[7, 3] = -1.0            # G <= 0
    theta[9, 4] = np.nan
    if sample_sd:
        theta[11, -1] = 0.0       # sd <= 0
    bad = {7, 9, 11} if sample_sd else {7, 9}
    got = ref.pointwise(x, flux, noise, theta.reshape(12, 5, -1), 4, vo.MODE_VOIGT4, sample_sd)
    L = np.longdouble
    ll = []
    for s in range(60):           # the double loop: every sample, every pixel
        if s in bad:
            continue
        taus = sum(vo.voigt_function(x, theta[s, 4 * k + 1], theta[s, 4 * k], theta[s, 4 * k + 2], theta[s, 4 * k + 3]) for k in range(4))
        row = []
        for p in range(x.size):
            sg = L(theta[s, -1]) if sample_sd else L(noise[p])
            row.append(-L(0.5) * ((L(flux[p]) - L(np.exp(-taus[p]))) / sg) ** 2 - np.log(sg) - L(0.5) * np.log(2 * L(np.pi)))
        ll.append(row)
    ll = np.array(ll, dtype=L)
    n = ll.shape[0]
    assert got["n_used"] == n == 60 - len(bad) and got["n_bad"] == len(bad)
    m = ll.max(axis=0)
    want = {"lppd": m + np.log(np.exp(ll - m).sum(axis=0) / n), "ll_mean": ll.sum(axis=0) / n}
    want["p_waic_pix"] = ((ll - want["ll_mean"]) ** 2).sum(axis=0) / (n - 1)
    elpd = want["lppd"] - want["p_waic_pix"]
    want.update(elpd_waic=elpd.sum(), p_waic=want["p_waic_pix"].sum(), lnl_mean=want["ll_mean"].sum())
    b = ref.bars(got)
    # float64 sums of n = 57 terms err by at most a few n 2^-53 of their size: two orders inside the bars
    for k in ("lppd", "ll_mean", "p_waic_pix", "elpd_waic", "p_waic", "lnl_mean"):
        ratio = np.max(np.abs(np.asarray(got[k], dtype=L) - want[k]) / b[k])
        print(k, "error / bar", float(ratio))
        assert ratio <= 1e-2, (k, float(ratio))
    se = np.sqrt(x.size * ((elpd - elpd.mean()) ** 2).sum() / (x.size - 1))
    assert abs(got["elpd_se"] - float(se)) <= 1e-11 * float(se)
    assert got["n_high"] == int((want["p_waic_pix"] > 0.4).sum())


def test_all_bad_ensemble_is_nan_not_an_error():
    x, flux, noise, _ = _golden("H1215_r0_K2_m0_sd0")
    chain = np.ones((3, 4, 6))
    chain[:, :, 2] = 0.0          # sigma <= 0 everywhere
    got = ref.pointwise(x, flux, noise, chain, 2, vo.MODE_GAUSS3, False)
    assert got["n_used"] == 0 and got["n_bad"] == 12 and got["n_high"] == 0
    for k in ref.PIX + ref.GRP:
        assert np.isnan(got[k]).all(), k


def test_one_sample_chain():
    x, flux, noise, theta = _ball_case(42, 1, True, "H1215_r0_K2_m0_sd0", 2, 0)
    got = ref.pointwise(x, flux, None, theta.reshape(1, 1, -1), 2, vo.MODE_GAUSS3, True)
    ll = ref.loglik(x, flux, None, theta, 2, vo.MODE_GAUSS3, True)[0][0]
    np.testing.assert_array_equal(got["lppd"], ll)
    np.testing.assert_array_equal(got["ll_mean"], ll)
    assert np.isnan(got["p_waic_pix"]).all() and np.isnan(got["elpd_waic"]) and np.isnan(got["p_waic"]) and got["n_used"] == 1
    assert got["lnl_mean"] == pytest.approx(ll.sum(), rel=1e-14)


def test_minus_infinity_follows_numpy():
    x, flux, noise, theta = _ball_case(43, 6, True, "H1215_r0_K2_m0_sd0", 2, 0)
    theta[2, -1] = 1e-200         # the residual over sd overflows when squared: l = -inf
    got = ref.pointwise(x, flux, None, theta.reshape(3, 2, -1), 2, vo.MODE_GAUSS3, True)
    assert got["n_bad"] == 0 and np.isfinite(got["lppd"]).all()
    assert np.isneginf(got["ll_mean"]).all() and np.isnan(got["p_waic_pix"]).all()


# ---- the planted errors the GPU comparison must see ----------------------------------------------------------
def _planted(ll, sigma, which):
    n, P = ll.shape
    if which == "dropped 65th sample":
        return ref.column_stats(np.delete(ll, 64, axis=0))
    if which == "ln sigma left out":
        return ref.column_stats(ll + np.log(sigma))
    lppd, mean, pw = ref.column_stats(ll)
    if which == "ddof 0":
        return lppd, mean, pw * (n - 1) / n
    if which == "mean for log-mean-exp":
        return mean, mean, pw
    raise AssertionError(which)


@pytest.mark.parametrize("sample_sd", [False, True])
@pytest.mark.parametrize("which", ["dropped 65th sample", "ln sigma left out", "ddof 0", "mean for log-mean-exp"])
def test_planted_errors_miss_the_bars_by_orders_of_magnitude(which, sample_sd):
    """on a ball chain of 129 samples -- the kind the GPU tests use -- each planted error is at least 1e3 bars away in a
    per-pixel statistic and in a group sum"""
    x, flux, noise, theta = _ball_case(44, 129, sample_sd)
    want = ref.pointwise(x, flux, noise, theta.reshape(129, 1, -1), 4, vo.MODE_VOIGT4, sample_sd)
    assert want["n_bad"] == 0
    ll, _, sigma, _ = ref.loglik(x, flux, noise, theta, 4, vo.MODE_VOIGT4, sample_sd)
    lppd, mean, pw = _planted(ll, np.broadcast_to(sigma, ll.shape), which)
    got = {"lppd": lppd, "ll_mean": mean, "p_waic_pix": pw, **ref.totals(lppd, pw, mean), "n_used": 129, "n_bad": 0}
    b = ref.bars(want)
    pix = max(float(np.max(np.abs(got[k] - want[k]) / b[k])) for k in ref.PIX)
    grp = max(abs(got[k] - want[k]) / b[k] for k in ("elpd_waic", "p_waic", "lnl_mean"))
    print(which, "worst per-pixel error / bar %.3g, worst group error / bar %.3g" % (pix, grp))
    assert pix >= 1e3 and grp >= 1e3
    with pytest.raises(AssertionError):
        ref.check(got, want)


# ---- the library boundary ----------------------------------------------------------------------------------
def _header_src(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_functions(stem="pred"):
    return sorted(set(re.findall(r"\b(vamp_%s[a-z0-9_]+)\s*\(" % ("" if stem == "hip" else stem + "_"), _header_src("vamp_%s.h" % stem))))


@pytest.fixture(scope="module")
def pred_lib():
    import vamp_amd.build as vb
    return vb.build_pred(verbose=False)


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out)))


def test_pred_library_builds_and_exports_the_header(pred_lib):
    assert os.path.exists(pred_lib)
    names = _header_functions()
    assert names == ["vamp_pred_last_error", "vamp_pred_pointwise", "vamp_pred_version"]
    assert _exports(pred_lib) == names


def test_build_makes_five_libraries_and_leaves_the_other_four_alone():
    import vamp_amd.build as vb
    assert vb.build(verbose=False).endswith("libvamp_hip.so")
    for stem in ("hip", "diag", "post", "evid", "pred"):
        path = os.path.join(ROOT, "vamp_amd", "libvamp_%s.so" % stem)
        assert os.path.exists(path), stem
        assert _exports(path) == _header_functions(stem), stem           # nm -D: what each header declares, nothing of another
    assert set(vb.PRED_DEPS) == {vb.PRED_SRC, os.path.join(vb.HERE, "csrc", "voigt_math.hpp"), os.path.join(vb.HERE, "csrc", "side_call.hpp"),
                                 os.path.join(vb.HERE, "csrc", "lane_group.hpp"), os.path.join(vb.HERE, "csrc", "chain_groups.hpp"),
                                 os.path.join(vb.HERE, "csrc", "pointwise_ll.hpp"), os.path.join(vb.HERE, "..", "include", "vamp_pred.h")}
    assert vb.PRED_FLAGS == vb.POST_FLAGS and "-fvisibility=hidden" in vb.PRED_FLAGS
    for name in ("vamp_hip.h", "vamp_diag.h", "vamp_post.h", "vamp_evid.h"):
        assert "vamp_pred" not in open(os.path.join(ROOT, "include", name)).read()
    assert re.search(r"#define VAMP_ABI_VERSION 4\b", open(os.path.join(ROOT, "include", "vamp_hip.h")).read())


_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const char*": C.c_char_p,
           "const double* const*": C.POINTER(C.c_void_p), "double*": C.POINTER(C.c_double),
           "const int64_t*": C.POINTER(C.c_int64), "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32)}


def _header_prototypes():
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(vamp_pred_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_src("vamp_pred.h")):
        types_ = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm in ("void", ""):
                continue
            types_.append(re.sub(r"\s*\*", "*", re.sub(r"\s*\b\w+$", "", prm)))
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types_)
    return protos


def test_pred_ctypes_table_mirrors_header():
    from vamp_amd import _pred_lib
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(_pred_lib.SIGNATURES)
    assert len(protos["vamp_pred_pointwise"][1]) == 26 and protos["vamp_pred_pointwise"][1][12] == "const int64_t*"
    assert protos["vamp_pred_pointwise"][1][15] == "int64_t"
    for name, (ret, params) in protos.items():
        res, args = _pred_lib.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(args) == len(params), name
        for i, (ty, arg) in enumerate(zip(params, args)):
            assert arg is _CTYPES[ty] or arg == _CTYPES[ty], (name, i, ty, arg)


def test_limits_are_the_posterior_library_s():
    from vamp_amd import posterior, predictive
    src = open(os.path.join(ROOT, "include", "vamp_pred.h")).read()
    assert re.search(r"#define VAMP_PRED_MAX_SAMPLES 16384\b", src) and re.search(r"#define VAMP_PRED_MAX_COMPONENTS 32\b", src)
    assert predictive.MAX_SAMPLES == posterior.MAX_SAMPLES == 16384 and predictive.time_step is posterior.time_step


def test_arguments_are_checked_before_any_device_call(pred_lib):
    from vamp_amd import _pred_lib, predictive
    lib = _pred_lib.load()
    assert lib.vamp_pred_version() == 1
    x = np.linspace(-3.0, 3.0, 7)
    y, nz = np.ones(7), np.full(7, 0.1)
    chain = np.ones((10, 4, 7))

    def call(n=10, W=4, K=2, mode=0, sd=0, ld=28, base=chain.ctypes.data, xs=x, flux=y, noise=nz, scratch=0):
        with pytest.raises(_pred_lib.PredError) as e:
            predictive._call(0, [xs], [flux], [noise], [K], [mode], [sd], [base], False, [ld], [n], [W], scratch)
        return str(e.value)

    assert "noise must be NULL" in call(sd=1)
    assert "NULL noise" in call(noise=None)
    bad = y.copy()
    bad[2] = np.nan
    assert "flux is not finite at pixel 2" in call(flux=bad)
    bad = y.copy()
    bad[6] = np.inf
    assert "flux is not finite at pixel 6" in call(flux=bad, noise=None, sd=1)
    for v in (0.0, -0.1, np.nan, np.inf):
        bad = nz.copy()
        bad[4] = v
        assert "noise is not finite and positive at pixel 4" in call(noise=bad)
    assert "exceeds 16384" in call(n=16385, W=1, ld=6)
    assert "exceeds 16384" in call(n=128, W=129, ld=129 * 6)
    assert "NBZ3" in call(mode=2)
    assert "mode must be" in call(mode=3)
    assert "n_comp = 0" in call(K=0)
    assert "n_comp = 33" in call(K=33, ld=4 * 99)
    assert "ld < walkers * ndim" in call(ld=23)
    assert "ld < walkers * ndim" in call(sd=1, noise=None, ld=27)          # D = 7 with the free sd
    bad_x = x.copy()
    bad_x[3] = np.inf
    assert "abscissa is not finite at pixel 3" in call(xs=bad_x)
    assert "NULL base" in call(base=0)
    assert "less than one column" in call(scratch=8 * 40 - 1)
    assert lib.vamp_pred_pointwise(0, None, 0, *([None] * 7), None, 0, *([None] * 3), 0, *([None] * 10)) == -1
    assert b"n_groups" in lib.vamp_pred_last_error()
    with pytest.raises(ValueError):
        predictive.pointwise_predictive(x, y, nz, np.zeros((4, 4)), 1, 0)
    with pytest.raises(ValueError):
        predictive.pointwise_predictive(x, y, None, np.zeros((4, 4, 3)), 1, 0)      # free sd: a Gaussian line has 4 parameters


def test_compare_is_its_formula():
    from vamp_amd import predictive
    rng = np.random.default_rng(45)
    a, b = types.SimpleNamespace(elpd=rng.normal(size=23)), types.SimpleNamespace(elpd=rng.normal(size=23))
    d = b.elpd - a.elpd
    diff, se = predictive.compare(a, b)
    assert diff == pytest.approx(d.sum(), rel=1e-14)
    assert se == pytest.approx(np.sqrt(23 * ((d - d.mean()) ** 2).sum() / 22), rel=1e-13)
    back = predictive.compare(b, a)
    assert back[0] == pytest.approx(-diff, rel=1e-14) and back[1] == pytest.approx(se, rel=1e-14)
    with pytest.raises(ValueError):
        predictive.compare(a, types.SimpleNamespace(elpd=np.zeros(22)))


# ---- wiring, with the library call replaced by the restatement ------------------------------------------------
@pytest.fixture
def fake_library(monkeypatch):
    from vamp_amd import predictive
    calls = []
    monkeypatch.setattr(predictive, "_pred_host", ref.fake_pred_host(calls))
    return calls


def _fake_fit(x, flux, noise, chain, K, mode):
    from vamp_amd.vpfits import _EnsembleMCMC
    fit = types.SimpleNamespace(_chain_dev=chain, _x=np.asarray(x), _flux=np.asarray(flux), noise=noise, _n=K, _mode=mode,
                                _sample_sd=noise is None, device=0)
    mc = _EnsembleMCMC(fit)
    mc._flat = chain.reshape(-1, chain.shape[2])
    fit.mcmc = mc
    return fit


def _chain(rng, x, K, mode, N, W, sample_sd):
    return pref.draw_prior(rng, x, K, mode, N * W, sample_sd).reshape(N, W, -1)


def test_waic_is_cached(fake_library):
    x, flux, noise, _ = _golden("H1215_r0_K2_m0_sd0")
    rng = np.random.default_rng(46)
    chain = _chain(rng, x, 2, 0, 9, 6, True)
    fit = _fake_fit(x, flux, None, chain, 2, 0)
    rec = fit.mcmc.waic()
    assert fake_library == [(1, [1])] and fit.mcmc.waic() is rec and fake_library == [(1, [1])]
    want = ref.pointwise(x, flux, None, chain, 2, 0, True)
    for k in ref.PIX:
        np.testing.assert_array_equal(getattr(rec, k), want[k])
    np.testing.assert_array_equal(rec.elpd, want["lppd"] - want["p_waic_pix"])
    assert rec.elpd_waic == want["elpd_waic"] and rec.waic == -2.0 * want["elpd_waic"] and rec.elpd_se == want["elpd_se"]
    assert (rec.p_waic, rec.lnl_mean, rec.n_high, rec.n_used, rec.n_bad, rec.step) == (want["p_waic"], want["lnl_mean"], want["n_high"], 54, 0, 1)
    known = _fake_fit(x, flux, noise, chain[:, :, :6].copy(), 2, 0)
    assert known.mcmc.waic().elpd_waic == ref.pointwise(x, flux, noise, chain[:, :, :6], 2, 0, False)["elpd_waic"]
    none = _fake_fit(x, flux, None, chain, 2, 0)
    none._chain_dev = None
    with pytest.raises(RuntimeError):
        none.mcmc.waic()


def test_fits_predictive_one_call_and_the_time_step(fake_library):
    from vamp_amd import predictive
    x, flux, noise, _ = _golden("H1215_r0_K2_m0_sd0")
    rng = np.random.default_rng(47)
    short = _fake_fit(x, flux, noise, _chain(rng, x, 1, 1, 5, 4, False), 1, 1)
    long_ = _fake_fit(x[:9], flux[:9], None, _chain(rng, x[:9], 1, 0, 700, 64, True), 1, 0)      # 44 800 samples: every third time
    none = types.SimpleNamespace(mcmc=None, _chain_dev=None)
    have, recs = predictive.fits_predictive([short, none, long_])
    assert fake_library == [(2, [1, 3])] and have == [short, long_]
    assert [r.step for r in recs] == [1, 3]
    want = ref.pointwise(x[:9], flux[:9], None, long_._chain_dev[::3], 1, 0, True)
    assert recs[1].n_used + recs[1].n_bad == 234 * 64
    np.testing.assert_array_equal(recs[1].lppd, want["lppd"])
    assert long_.mcmc.waic() is recs[1] and fake_library == [(2, [1, 3])]           # the one call filled each fit's cache


def _fake_spectrum(rng, tmp_path=None, VPspectrum=None):
    if VPspectrum is None:
        from vamp_amd.vpspectrum import VPspectrum
    lam = np.linspace(1210.0, 1220.0, 120)
    pixels = [(10, 30), (50, 94)]
    spec = VPspectrum.__new__(VPspectrum)
    spec.wavelength_array, spec.flux_array, spec.region_pixels, spec.device = lam, np.ones(120), pixels, 0
    spec.regions = []
    for (s, e), K in zip(pixels, (1, 2)):
        P = e - s
        x = np.arange(P) - 0.5 * (P - 1)
        flux = 1.0 - 0.3 * np.exp(-0.5 * (x / 3.0) ** 2) + 0.01 * rng.standard_normal(P)
        spec.regions.append(types.SimpleNamespace(fit=_fake_fit(x, flux, None, _chain(rng, x, K, 0, 6, 8, True), K, 0), n=K, num_pixels=P,
                                                  best_chi_squared=1.0))
    if tmp_path is not None:
        spec.output_filename = str(tmp_path / "spectrum_9_gauss_")
    return spec


def test_spectrum_predictive_layout(fake_library):
    rng = np.random.default_rng(48)
    spec = _fake_spectrum(rng)
    pred = spec.predictive()
    assert fake_library == [(2, [1, 1])]                           # one call over the kept fits
    assert set(pred) == {"lppd", "ll_mean", "p_waic_pix", "elpd", "elpd_waic", "elpd_se", "p_waic", "waic", "lnl_mean", "n_high",
                         "n_used", "n_bad", "n_comp", "time_step"}
    outside = np.ones(120, bool)
    for j, (s, e) in enumerate(spec.region_pixels):
        outside[s:e] = False
        fit = spec.regions[j].fit
        want = ref.pointwise(fit._x, fit._flux, None, fit._chain_dev, fit._n, 0, True)
        for k in ref.PIX:
            assert pred[k].shape == (120,)
            np.testing.assert_array_equal(pred[k][s:e], want[k][::-1])      # flipped like _harvest
        np.testing.assert_array_equal(pred["elpd"][s:e], (want["lppd"] - want["p_waic_pix"])[::-1])
        assert pred["elpd_waic"][j] == want["elpd_waic"] and pred["waic"][j] == -2 * want["elpd_waic"]
        assert pred["elpd_se"][j] == want["elpd_se"] and pred["n_used"][j] == want["n_used"] and pred["n_high"][j] == want["n_high"]
    for k in ref.PIX + ("elpd",):
        assert np.isnan(pred[k][outside]).all()
    assert list(pred["n_comp"]) == [1, 2] and list(pred["time_step"]) == [1, 1]
    spec.regions[1].fit._chain_dev = None
    with pytest.raises(RuntimeError):
        spec.predictive()


def test_do_vamp_predictive_is_opt_in(fake_library, monkeypatch, tmp_path, capsys):
    """the record field and the file only with --predictive; without it the record has exactly the fields it had"""
    from vamp_amd import diagnostics, do_vamp, h5min, vpspectrum
    rng = np.random.default_rng(49)
    made, real = [], vpspectrum.VPspectrum

    class Spec:
        def __new__(cls, *a, **kw):
            spec = _fake_spectrum(rng, tmp_path, real)
            spec.chi_limit, spec.flux_model, spec.voigt, spec.dtype = 1.5, {"difficult_fit": False}, False, 0
            spec.fit_spectrum = lambda batched=False: {}
            made.append(spec)
            return spec

    monkeypatch.setattr(vpspectrum, "VPspectrum", Spec)
    monkeypatch.setattr(diagnostics, "fits_diagnostics", lambda fits, device=0: ([], 0))
    recs = []
    for flags in ([], ["--predictive"]):
        assert do_vamp.main([__file__, "1215.67", "--output_folder", str(tmp_path)] + flags) == 0
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("vamp_perf ")]
        recs.append(json.loads(line[0][len("vamp_perf "):]))
        assert os.path.exists(tmp_path / "spectrum_9_gauss_predictive.h5") == bool(flags)
    assert set(recs[1]) - set(recs[0]) == {"predictive_seconds"} and set(recs[0]) <= set(recs[1])
    assert fake_library == [(2, [1, 1])] and recs[1]["predictive_seconds"] >= 0
    back = h5min.read(str(tmp_path / "spectrum_9_gauss_predictive.h5"))
    want = made[1].predictive()
    assert set(back) == set(want)
    for k in want:
        np.testing.assert_array_equal(back[k], want[k])
        assert back[k].dtype == want[k].dtype, k


# ---- the ladder, with planted records -------------------------------------------------------------------------
def _ladder_region(monkeypatch, planted, calls):
    """a VPregion whose ``_fit_n`` makes chain-carrying stand-ins; their records are the restatement's with ``planted``
    per-pixel elpd"""
    from vamp_amd import predictive
    from vamp_amd.vpregion import VPregion
    monkeypatch.setattr(predictive, "_pred_host", ref.fake_pred_host(calls, planted))
    x = np.arange(20) - 9.5
    flux = 1.0 - 0.4 * np.exp(-0.5 * (x / 2.0) ** 2)
    region = VPregion(1e15 + 1e10 * x, flux, np.full(20, 0.05), seed=3, nwalkers=8)
    assert region.n == 1
    rng = np.random.default_rng(50)
    built, closed = [], []

    def fit_n(n, iterations, thin, burn):
        fit = _fake_fit(x, flux, None, _chain(rng, x, n, 0, 4, 8, True), n, 0)
        fit._ctx = types.SimpleNamespace(close=lambda n=n: closed.append(n))
        fit.bic_array, fit.red_chi_array = [10.0 * n] * 3, [5.0] * 3
        fit._run_sampler = lambda *a, n=n: built.append(("sampled from the MAP", n) + a)
        fit.map = types.SimpleNamespace(fit=lambda n=n, **kw: built.append(("polished", n)))
        built.append(n)
        return fit

    region._fit_n = fit_n
    return region, built, closed


def test_waic_ladder_adds_a_line_at_rise_above_se_and_stops_at_rise_below(monkeypatch):
    from vamp_amd import predictive
    wiggle = np.where(np.arange(20) % 2 == 0, 1.0, -0.9)          # sum 1.0, paired se 4.4
    elpd = {1: np.zeros(20), 2: np.full(20, 0.5) + 0.01 * np.arange(20), 3: np.full(20, 0.5) + 0.01 * np.arange(20) + wiggle}
    calls = []
    region, built, closed = _ladder_region(monkeypatch, lambda k: elpd[k], calls)
    region.region_fit(verbose=False, iterations=10, thin=1, burn=0, criterion='waic')
    rung = lambda n: [n, ("sampled from the MAP", n, 10, 0, 1), ("polished", n)]      # find_bic's chain precedes its MAP
    assert built == rung(1) + rung(2) + rung(3) and region.n == 2 and region.fit._n == 2
    assert closed == [1, 3]                                        # the dropped fits are released, the kept one is not
    assert sorted(region.predictive) == [1, 2, 3] and region.fit.predictive is region.predictive[2]
    assert [c[0] for c in calls] == [1, 1, 1]                      # one library call per rung
    up, se_up = predictive.compare(region.predictive[1], region.predictive[2])
    flat_, se_flat = predictive.compare(region.predictive[2], region.predictive[3])
    assert up > se_up and up == pytest.approx(11.9) and flat_ == pytest.approx(1.0) and 4.0 < se_flat < 5.0 and not flat_ > se_flat
    # a rise inside the standard error at the first rung: the first fit is kept
    first = {1: np.zeros(20), 2: wiggle}
    region, built, closed = _ladder_region(monkeypatch, lambda k: first[k], [])
    region.region_fit(verbose=False, criterion='waic')
    assert region.n == 1 and region.fit._n == 1 and [b for b in built if isinstance(b, int)] == [1, 2] and closed == [2]
    assert region.fit.predictive is region.predictive[1]


def test_bic_ladder_makes_no_predictive_call(monkeypatch):
    calls = []
    region, built, closed = _ladder_region(monkeypatch, None, calls)
    region.region_fit(verbose=False, iterations=10, thin=1, burn=0)
    assert built == [1, 2] and region.n == 1 and calls == [] and not hasattr(region, "predictive")
    with pytest.raises(ValueError, match="'bic', 'evidence' or 'waic'"):
        region.region_fit(verbose=False, criterion='aic')
