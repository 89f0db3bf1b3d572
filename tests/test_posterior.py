"""CPU tests of the posterior summaries: the numpy restatement (tests/posterior_ref.py) against a brute-force
loop and the physics module's equivalent widths, the libvamp_post.so boundary (build, exports, ctypes table, argument
checks before any device call), and the Python wiring (mcmc.flux_band / equivalent_widths, fits_posterior's time step,
VPspectrum.posterior_summaries, do_vamp --posterior) with the library call replaced by the restatement."""
import ctypes as C
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

import posterior_ref as ref
from conftest import ROOT, load_golden
from oracle import vamp_oracle as vo

PROBS = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0)


def _golden(name="H1215_r0_K4_m1_sd0"):
    g = load_golden("lnprob_cases.npz")
    return g[name + "_x"], g[name + "_theta"]


# ---- the restatement ---------------------------------------------------------------------------------------
def test_restatement_against_a_brute_force_loop():
    x, th = _golden()
    rng = np.random.default_rng(31)
    theta = ref.ball(rng, th[np.isfinite(load_golden("lnprob_cases.npz")["H1215_r0_K4_m1_sd0_lnprob"])][0], 12 * 5)
    theta[7, 3] = -1.0            # G <= 0
    theta[9, 4] = np.nan
    theta[11, 2] = -0.5           # L < 0
    chain = theta.reshape(12, 5, 16)
    got = ref.summaries(x, chain, 4, vo.MODE_VOIGT4, probs=PROBS, pixel_width=0.25)
    flux, ew, cew = [], [], []
    for s in range(60):           # the three-line loop: tau of every line, flux, decrement sums
        if s in (7, 9, 11):
            continue
        taus = np.array([vo.voigt_function(x, theta[s, 4 * k + 1], theta[s, 4 * k], theta[s, 4 * k + 2], theta[s, 4 * k + 3]) for k in range(4)])
        flux.append(np.exp(-taus.sum(0))); ew.append(0.25 * np.sum(1 - flux[-1])); cew.append(0.25 * np.sum(1 - np.exp(-taus), axis=1))
    flux, ew, cew = np.array(flux), np.array(ew), np.array(cew)
    assert got["n_used"] == 57 and got["n_bad"] == 3
    np.testing.assert_allclose(got["flux_mean"], flux.mean(0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(got["flux_sd"], flux.std(0), rtol=0, atol=1e-14)
    for i, p in enumerate(PROBS):
        np.testing.assert_allclose(got["flux_q"][i], [np.quantile(flux[:, j], p) for j in range(x.size)], rtol=0, atol=1e-14)
        assert got["ew_q"][i] == pytest.approx(np.quantile(ew, p), abs=1e-13)
        np.testing.assert_allclose(got["comp_ew_q"][:, i], [np.quantile(cew[:, k], p) for k in range(4)], rtol=0, atol=1e-13)
    assert got["ew_mean"] == pytest.approx(ew.mean(), abs=1e-13) and got["ew_sd"] == pytest.approx(ew.std(), abs=1e-13)
    np.testing.assert_allclose(got["comp_ew_mean"], cew.mean(0), rtol=0, atol=1e-13)
    np.testing.assert_allclose(got["comp_ew_sd"], cew.std(0), rtol=0, atol=1e-13)
    assert got["flux_q"][0].max() <= got["flux_q"][3].min() + 1 and np.all(np.diff(got["flux_q"], axis=0) >= 0)


def test_all_bad_ensemble_is_nan_not_an_error():
    x, _ = _golden("H1215_r0_K2_m0_sd0")
    chain = np.ones((3, 4, 6))
    chain[:, :, 2] = 0.0          # sigma <= 0 everywhere
    got = ref.summaries(x, chain, 2, vo.MODE_GAUSS3, probs=PROBS)
    assert got["n_used"] == 0 and got["n_bad"] == 12
    assert np.isnan(got["flux_mean"]).all() and np.isnan(got["flux_q"]).all() and np.isnan(got["ew_mean"])
    assert np.isnan(got["comp_ew_q"]).all() and got["comp_ew_q"].shape == (2, len(PROBS))


@pytest.mark.parametrize("mode", [vo.MODE_GAUSS3, vo.MODE_VOIGT4])
def test_single_sample_ew_is_the_physics_module_s(mode):
    """EW of one sample = EquivalentWidthFlux of its flux, a line's = EquivalentWidthTau of its tau, with edges whose
    mean spacing is the pixel width"""
    from vamp_amd import physics
    x, _ = _golden("H1215_r0_K2_m0_sd0")
    rng = np.random.default_rng(32)
    theta = ref.draw_prior(rng, x, 2, mode, 1)
    lam = np.linspace(1215.0, 1217.5, x.size)
    width = abs(lam[-1] - lam[0]) / (x.size - 1)
    got = ref.summaries(x, theta.reshape(1, 1, -1), 2, mode, probs=(0.5,), pixel_width=width)
    tau = ref.sample_taus(x, theta, 2, mode)[0]
    assert got["ew_mean"] == pytest.approx(physics.EquivalentWidthFlux(np.exp(-tau.sum(0)), lam), rel=1e-13)
    assert got["ew_q"][0] == got["ew_mean"] and got["ew_sd"] == 0.0
    for k in range(2):
        assert got["comp_ew_mean"][k] == pytest.approx(physics.EquivalentWidthTau(tau[k], lam), rel=1e-13)


# ---- the library boundary ----------------------------------------------------------------------------------
def _header_src(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_functions():
    return sorted(set(re.findall(r"\b(vamp_post_[a-z0-9_]+)\s*\(", _header_src("vamp_post.h"))))


@pytest.fixture(scope="module")
def post_lib():
    import vamp_amd.build as vb
    return vb.build_post(verbose=False)


def test_post_library_builds_and_exports_the_header(post_lib):
    assert os.path.exists(post_lib)
    names = _header_functions()
    assert names == ["vamp_post_last_error", "vamp_post_summaries", "vamp_post_version"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", post_lib], text=True)
    assert sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out))) == names


_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const char*": C.c_char_p,
           "const double* const*": C.POINTER(C.c_void_p), "double*": C.POINTER(C.c_double), "const double*": C.POINTER(C.c_double),
           "const int64_t*": C.POINTER(C.c_int64), "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32)}


def _header_prototypes():
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(vamp_post_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_src("vamp_post.h")):
        types_ = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm in ("void", ""):
                continue
            types_.append(re.sub(r"\s*\*", "*", re.sub(r"\s*\b\w+$", "", prm)))
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types_)
    return protos


def test_post_ctypes_table_mirrors_header():
    from vamp_amd import _post_lib
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(_post_lib.SIGNATURES)
    assert protos["vamp_post_summaries"][1][10] == "const int64_t*" and protos["vamp_post_summaries"][1][16] == "int64_t"
    for name, (ret, params) in protos.items():
        res, args = _post_lib.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(args) == len(params), name
        for i, (ty, arg) in enumerate(zip(params, args)):
            assert arg is _CTYPES[ty] or arg == _CTYPES[ty], (name, i, ty, arg)


def test_main_library_abi_untouched():
    """the summaries live in their own library: vamp_hip.h, its ctypes table and libvamp_hip.so's exports do not name
    them, and the ABI version is what it was"""
    import vamp_amd.build as vb
    from vamp_amd import _diag_lib, _lib
    assert not any("post" in n for n in list(_lib.SIGNATURES) + list(_diag_lib.SIGNATURES))
    main = open(os.path.join(ROOT, "include", "vamp_hip.h")).read()
    assert "vamp_post" not in main and re.search(r"#define VAMP_ABI_VERSION 4\b", main)
    assert "vamp_post" not in open(os.path.join(ROOT, "include", "vamp_diag.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", vb.build(verbose=False)], text=True)
    exported = sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out)))
    assert exported == sorted(set(re.findall(r"\b(vamp_[a-z0-9_]+)\s*\(", _header_src("vamp_hip.h"))))
    assert vb.build(verbose=False).endswith("libvamp_hip.so")


def test_arguments_are_checked_before_any_device_call(post_lib):
    from vamp_amd import _post_lib, posterior
    lib = _post_lib.load()
    assert lib.vamp_post_version() == 1
    x = np.linspace(-3.0, 3.0, 7)
    chain = np.ones((10, 4, 6))

    def call(n=10, W=4, K=2, mode=0, sd=0, ld=24, base=chain.ctypes.data, xs=x, probs=(0.5,), scratch=0, width=1.0):
        with pytest.raises(_post_lib.PostError) as e:
            posterior._call(0, [xs], [K], [mode], [sd], [base], False, [ld], [n], [W], [width], probs, scratch)
        return str(e.value)

    assert "exceeds 16384" in call(n=16385, W=1, ld=6)
    assert "exceeds 16384" in call(n=128, W=129, ld=129 * 6)
    assert "n_comp = 0" in call(K=0)
    assert "n_comp = 33" in call(K=33, ld=4 * 99)
    assert "NBZ3" in call(mode=2)
    assert "mode must be" in call(mode=3)
    assert "n_probs = 0" in call(probs=np.zeros(0))
    assert "n_probs = 17" in call(probs=np.linspace(0, 1, 17))
    assert "probs[1] is outside" in call(probs=(0.5, 1.5))
    assert "probs[0] is outside" in call(probs=(-0.1,))
    assert "probs[2] is outside" in call(probs=(0.1, 0.2, np.nan))
    assert "ld < walkers * ndim" in call(ld=23)
    assert "ld < walkers * ndim" in call(sd=1, ld=27)          # D = 7 with the free sd
    bad_x = x.copy()
    bad_x[3] = np.inf
    assert "not finite at pixel 3" in call(xs=bad_x)
    assert "NULL base" in call(base=0)
    assert "less than one column" in call(scratch=8 * 40 - 1)
    assert "pixel_width" in call(width=np.nan)
    assert lib.vamp_post_summaries(0, None, 0, *([None] * 5), None, 0, *([None] * 4), 1, None, 0, *([None] * 11)) == -1
    assert b"n_groups" in lib.vamp_post_last_error()
    with pytest.raises(ValueError):
        posterior.posterior_summaries(x, np.zeros((4, 4)), 1, 0)
    with pytest.raises(ValueError):
        posterior.posterior_summaries(x, np.zeros((4, 4, 5)), 1, 0)      # 5 parameters are not one Gaussian line


# ---- wiring, with the library call replaced by the restatement ------------------------------------------------
@pytest.fixture
def fake_library(monkeypatch):
    from vamp_amd import posterior
    calls = []
    monkeypatch.setattr(posterior, "_post_host", ref.fake_post_host(calls))
    return calls


def _fake_fit(x, chain, K, mode, sample_sd=False):
    from vamp_amd.vpfits import _EnsembleMCMC
    fit = types.SimpleNamespace(_chain_dev=chain, _x=np.asarray(x), _n=K, _mode=mode, _sample_sd=sample_sd, device=0)
    mc = _EnsembleMCMC(fit)
    mc._flat = chain.reshape(-1, chain.shape[2])
    q = 4 if mode == 1 else 3
    mc._names = ["p%d" % i for i in range(q * K)] + (["sd"] if sample_sd else [])
    fit.mcmc = mc
    return fit


def _chain(rng, x, K, mode, N, W, sample_sd=False):
    return ref.draw_prior(rng, x, K, mode, N * W, sample_sd).reshape(N, W, -1)


def test_flux_band_and_equivalent_widths_are_cached(fake_library):
    x, _ = _golden("H1215_r0_K2_m0_sd0")
    rng = np.random.default_rng(33)
    chain = _chain(rng, x, 2, 0, 9, 6, sample_sd=True)
    fit = _fake_fit(x, chain, 2, 0, sample_sd=True)
    before = dict(fit.mcmc.stats()["p0"])
    band = fit.mcmc.flux_band()
    assert fake_library == [1]
    want = ref.summaries(x, chain, 2, 0, True)
    assert sorted(band) == ["mean", "quantiles", "sd"] and sorted(band["quantiles"]) == [0.025, 0.16, 0.5, 0.84, 0.975]
    np.testing.assert_array_equal(band["mean"], want["flux_mean"])
    np.testing.assert_array_equal(band["sd"], want["flux_sd"])
    np.testing.assert_array_equal(band["quantiles"][0.84], want["flux_q"][3])
    lam = np.linspace(1216.0, 1214.0, x.size)                  # descending, as a region's wavelengths are in the fit's order
    ew = fit.mcmc.equivalent_widths(lam)
    fit.mcmc.flux_band()
    assert fake_library == [1]                                  # both from one call per fit
    width = 2.0 / (x.size - 1)
    assert ew["pixel_width"] == pytest.approx(width) and ew["n_used"] == 54 and ew["n_bad"] == 0
    assert ew["EW"]["mean"] == pytest.approx(want["ew_mean"] * width, rel=1e-13)
    assert ew["EW"]["sd"] == pytest.approx(want["ew_sd"] * width, rel=1e-13)
    assert len(ew["components"]) == 2
    for k in range(2):
        assert ew["components"][k]["quantiles"][0.5] == pytest.approx(want["comp_ew_q"][k, 2] * width, rel=1e-13)
    fit.mcmc.flux_band(probs=(0.1, 0.9))
    assert fake_library == [1, 1]                               # other probabilities: another call, cached too
    fit.mcmc.equivalent_widths(lam, probs=(0.1, 0.9))
    assert fake_library == [1, 1]
    assert fit.mcmc.stats()["p0"] == before                     # stats() is what it was
    assert set(fit.mcmc.stats()["p0"]) == {"n", "standard deviation", "mean", "quantiles", "mc error"}


def test_fits_posterior_one_call_and_the_time_step(fake_library):
    from vamp_amd import posterior
    assert posterior.time_step(180, 64) == 1 and posterior.time_step(256, 64) == 1
    assert posterior.time_step(257, 64) == 2 and posterior.time_step(1000, 64) == 4 and posterior.time_step(3, 16384) == 3
    with pytest.raises(ValueError):
        posterior.time_step(10, 16385)
    x, _ = _golden("H1215_r0_K2_m0_sd0")
    rng = np.random.default_rng(34)
    short = _fake_fit(x, _chain(rng, x, 1, 1, 5, 4), 1, 1)
    long_ = _fake_fit(x[:9], _chain(rng, x[:9], 1, 0, 700, 64), 1, 0)          # 44 800 samples: every third time
    none = types.SimpleNamespace(mcmc=None, _chain_dev=None)
    have, recs = posterior.fits_posterior([short, none, long_])
    assert fake_library == [2] and have == [short, long_]
    assert [r.step for r in recs] == [1, 3]
    want = ref.summaries(x[:9], long_._chain_dev[::3], 1, 0)
    assert recs[1].n_used == 234 * 64
    np.testing.assert_array_equal(recs[1].flux_q, want["flux_q"])
    assert long_.mcmc.flux_band()["mean"] is not None and fake_library == [2]      # the one call filled each fit's cache


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
        spec.regions.append(types.SimpleNamespace(fit=_fake_fit(x, _chain(rng, x, K, 0, 6, 8), K, 0), n=K, num_pixels=P,
                                                  best_chi_squared=1.0))
    if tmp_path is not None:
        spec.output_filename = str(tmp_path / "spectrum_9_gauss_")
    return spec


def test_spectrum_posterior_summaries_layout(fake_library):
    rng = np.random.default_rng(35)
    spec = _fake_spectrum(rng)
    post = spec.posterior_summaries(probs=(0.16, 0.5, 0.84))
    assert fake_library == [2]                                  # one call over the kept fits
    assert set(post) == {"probs", "total_mean", "total_sd", "total_q", "EW_mean", "EW_sd", "EW_q", "line_EW_mean", "line_EW_sd",
                         "line_EW_q", "time_step"}
    assert post["total_q"].shape == (3, 120) and post["EW_q"].shape == (2, 3) and post["line_EW_q"].shape == (3, 3)
    outside = np.ones(120, bool)
    for j, (s, e) in enumerate(spec.region_pixels):
        outside[s:e] = False
        fit = spec.regions[j].fit
        lam = spec.wavelength_array[s:e]
        width = abs(lam[-1] - lam[0]) / (e - s - 1)
        want = ref.summaries(fit._x, fit._chain_dev, fit._n, 0, probs=(0.16, 0.5, 0.84), pixel_width=width)
        np.testing.assert_array_equal(post["total_mean"][s:e], want["flux_mean"][::-1])      # flipped like _harvest
        np.testing.assert_array_equal(post["total_q"][:, s:e], want["flux_q"][:, ::-1])
        assert post["EW_mean"][j] == want["ew_mean"] and np.array_equal(post["EW_q"][j], want["ew_q"])
    assert np.all(post["total_mean"][outside] == 1) and np.all(post["total_sd"][outside] == 0) and np.all(post["total_q"][:, outside] == 1)
    k2 = ref.summaries(spec.regions[1].fit._x, spec.regions[1].fit._chain_dev, 2, 0, probs=(0.16, 0.5, 0.84),
                       pixel_width=abs(spec.wavelength_array[93] - spec.wavelength_array[50]) / 43)
    np.testing.assert_array_equal(post["line_EW_mean"][1:], k2["comp_ew_mean"])            # the order of params['EW']


def test_do_vamp_posterior_is_opt_in(fake_library, monkeypatch, tmp_path, capsys):
    """the record field and the file only with --posterior; without it the record has exactly the fields it had"""
    from vamp_amd import diagnostics, do_vamp, h5min, vpspectrum
    rng = np.random.default_rng(36)
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
    for flags in ([], ["--posterior"]):
        assert do_vamp.main([__file__, "1215.67", "--output_folder", str(tmp_path)] + flags) == 0
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("vamp_perf ")]
        recs.append(json.loads(line[0][len("vamp_perf "):]))
        assert os.path.exists(tmp_path / "spectrum_9_gauss_posterior.h5") == bool(flags)
    assert set(recs[1]) - set(recs[0]) == {"posterior_seconds"} and set(recs[0]) <= set(recs[1])
    assert fake_library == [2] and recs[1]["posterior_seconds"] >= 0
    try:
        import h5py
        with h5py.File(tmp_path / "spectrum_9_gauss_posterior.h5", "r") as f:
            back = {k: f[k][()] for k in f}
    except ImportError:
        back = h5min.read(str(tmp_path / "spectrum_9_gauss_posterior.h5"))
    want = made[1].posterior_summaries()
    assert set(back) == set(want)
    for k in want:
        np.testing.assert_array_equal(back[k], want[k])
    assert json.load(open(str(tmp_path / "spectrum_9_gauss_perf.json"))) == recs[1]
