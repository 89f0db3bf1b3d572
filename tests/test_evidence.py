"""CPU tests of the log-evidence: the numpy restatement (tests/evidence_ref.py) -- its swap rule on a toy target, its
reductions, brute-force quadrature of ln Z --, the libvamp_evid.so boundary (build, exports, ctypes table, argument
checks before any device call), and the Python wiring (VPregion.region_fit(criterion=...), VPfit.log_evidence,
VPspectrum.evidences, do_vamp --evidence) with the library call replaced by a fake."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import evidence_ref as ref
from conftest import ROOT
from oracle import vamp_oracle as vo


# ---- the restatement ---------------------------------------------------------------------------------------
def test_swap_rule_leaves_a_two_rung_target_invariant():
    """two rungs over five states with likelihoods L: the joint target is L(s0)^b0 L(s1)^b1; with u on a fine grid the
    rule's acceptance is min(1, (L(s0) / L(s1))^(b1 - b0)), and the exchange it makes satisfies detailed balance"""
    lnl = np.log(np.array([0.02, 0.3, 1.0, 2.5, 40.0]))
    b0, b1 = 0.2, 0.7
    logu = np.log((np.arange(200000) + 0.5) / 200000)
    acc = np.array([[np.mean(ref.swap_rule(lnl[i], lnl[j], b1 - b0, logu)) for j in range(5)] for i in range(5)])
    want = np.minimum(1.0, np.exp((b1 - b0) * (lnl[:, None] - lnl[None, :])))
    np.testing.assert_allclose(acc, want, rtol=0, atol=1e-5)
    p = np.exp(b0 * lnl[:, None] + b1 * lnl[None, :])
    p /= p.sum()
    flow = p * acc                                   # probability flow (s0, s1) -> (s1, s0)
    np.testing.assert_allclose(flow, flow.T, rtol=1e-4)
    after = p - flow + flow.T                        # the distribution after one offered exchange
    np.testing.assert_allclose(after, p, rtol=1e-4)
    assert not ref.swap_rule(np.nan, 0.0, 0.5, -1.0) and not ref.swap_rule(-np.inf, -np.inf, 0.5, -1.0)      # NaN never swaps


def test_reductions_on_a_known_trace():
    """ln L ~ N(mu_j, s^2) per rung: log mean exp(db l) -> db mu + db^2 s^2 / 2; the blocks give a standard error"""
    rng = np.random.default_rng(1)
    betas = ref.default_betas(6)
    mu = np.linspace(-30.0, -5.0, 6)
    trace = mu[None, :, None] + 0.5 * rng.standard_normal((400, 6, 32))
    rec = ref.reduce(trace, betas)
    db = np.diff(betas)
    assert rec["lnZ"] == pytest.approx(np.sum(db * mu[:-1] + 0.5 * db ** 2 * 0.25), abs=0.02)
    assert 0 < rec["lnZ_se"] < 0.02
    assert rec["lnZ_ti"] == pytest.approx(np.sum(db * 0.5 * (mu[:-1] + mu[1:])), abs=0.02)
    np.testing.assert_allclose(rec["mean_lnL"], mu, atol=0.02)
    np.testing.assert_allclose(rec["var_lnL"], 0.25, atol=0.02)
    assert math.isnan(ref.reduce(trace[:7], betas)["lnZ_se"])
    assert ref.default_betas(16)[1] == pytest.approx((1 / 15) ** (1 / 0.3)) and ref.default_betas(2).tolist() == [0.0, 1.0]


def test_prior_draws_lie_inside_the_prior_and_follow_it():
    x = np.linspace(-4.0, 6.0, 11)
    for mode, sd in ((0, True), (1, False)):
        R = ref.make_region(x, np.ones(11), np.full(11, 0.1), 2, mode, sd)
        X = ref.prior_draws(R, 5, 400, 77)
        lp = np.array([vo.log_prior(R, t) for t in X])
        assert np.all(np.isfinite(lp))
        assert X[:, 0].mean() == pytest.approx(2.0, abs=0.25) and X[:, 1].mean() == pytest.approx(1.0, abs=0.6)      # Gamma(2, 1); U(-4, 6)
        assert not np.array_equal(X, ref.prior_draws(R, 6, 400, 77))


def test_quadrature_of_one_gaussian_line():
    """A = 1.2, c = 11.3, sigma = 2.5, noise 0.1, 24 pixels, numpy seed 3: the midpoint rule at 80^3 and 160^3 points"""
    x, flux, noise = ref.gauss_line_data(24, [(1.2, 11.3, 2.5)], 0.1, 3)
    z80, z160 = ref.quadrature_lnZ(x, flux, noise, 80), ref.quadrature_lnZ(x, flux, noise, 160)
    assert abs(z80 - z160) <= 0.01
    assert z80 == pytest.approx(8.227, abs=1e-3) and z160 == pytest.approx(8.227, abs=1e-3)
    # the integrand is the oracle's: one grid point against log_prior + log_like with the normalisation
    R = ref.make_region(x, flux, noise, 1, vo.MODE_GAUSS3)
    ll, lp = ref.lnlike_lnprior(R, np.array([1.2, 11.3, 2.5]))
    assert lp == pytest.approx(math.log(1.2) - 1.2 - math.log(23.0) - math.log(11.5), rel=1e-14)
    assert ll == pytest.approx(-0.5 * np.sum(((flux - np.exp(-vo.gauss_function(x, 1.2, 11.3, 2.5))) / 0.1) ** 2)
                               - 12 * math.log(2 * math.pi * 0.01), rel=1e-13)


def test_restatement_runs_a_short_ladder():
    x, flux, noise = ref.gauss_line_data(12, [(1.0, 5.0, 1.5)], 0.1, 8)
    R = ref.make_region(x, flux, noise, 1, vo.MODE_GAUSS3)
    a, b = (ref.run([R], [4], ref.default_betas(3), 6, 9, 1, 2, 99)[0] for _ in range(2))
    assert a["chain"].shape == (8, 6, 3) and a["lnl_trace"].shape == (8, 3, 6) and a["swap_trace"].shape == (4, 2, 6)
    assert np.array_equal(a["chain"], b["chain"]) and a["lnZ"] == b["lnZ"] and math.isfinite(a["lnZ_se"])
    assert np.array_equal(a["chain_lnl"], a["lnl_trace"][:, -1])
    assert a["swap_trace"][0, 1].sum() == 0 and a["swap_trace"][1, 0].sum() == 0         # even pairs, then odd pairs
    other = ref.run([R], [5], ref.default_betas(3), 6, 9, 1, 2, 99)[0]
    assert not np.array_equal(a["chain"], other["chain"])                                   # the region id keys the draws


# ---- the library boundary ----------------------------------------------------------------------------------
def _header_src(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_functions():
    return sorted(set(re.findall(r"\b(vamp_evid_[a-z0-9_]+)\s*\(", _header_src("vamp_evid.h"))))


@pytest.fixture(scope="module")
def evid_lib():
    import vamp_amd.build as vb
    return vb.build_evid(verbose=False)


def test_evid_library_builds_and_exports_the_header(evid_lib):
    assert os.path.exists(evid_lib)
    names = _header_functions()
    assert names == ["vamp_evid_default_betas", "vamp_evid_last_error", "vamp_evid_lnlike", "vamp_evid_run", "vamp_evid_version"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", evid_lib], text=True)
    assert sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out))) == names


def test_build_makes_four_libraries():
    import vamp_amd.build as vb
    assert vb.build(verbose=False).endswith("libvamp_hip.so")
    for name in ("libvamp_hip.so", "libvamp_diag.so", "libvamp_post.so", "libvamp_evid.so"):
        assert os.path.exists(os.path.join(ROOT, "vamp_amd", name)), name
    assert set(vb.EVID_DEPS) == {vb.EVID_SRC, os.path.join(vb.HERE, "csrc", "voigt_math.hpp"), os.path.join(vb.HERE, "csrc", "draws.hpp"),
                                 os.path.join(vb.HERE, "csrc", "side_call.hpp"), os.path.join(vb.HERE, "csrc", "lane_group.hpp"),
                                 os.path.join(vb.HERE, "..", "include", "vamp_evid.h")}
    assert vb.EVID_FLAGS == vb.POST_FLAGS


_CTYPES = {"int": C.c_int, "uint64_t": C.c_uint64, "double": C.c_double, "void*": C.c_void_p, "const char*": C.c_char_p,
           "const double* const*": C.POINTER(C.c_void_p), "double* const*": C.POINTER(C.c_void_p), "double*": C.POINTER(C.c_double),
           "const double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32), "uint8_t*": C.POINTER(C.c_uint8)}


def _header_prototypes():
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(vamp_evid_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_src("vamp_evid.h")):
        types_ = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm in ("void", ""):
                continue
            types_.append(re.sub(r"\s*\*", "*", re.sub(r"\s*\b\w+$", "", prm)))
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types_)
    return protos


def test_evid_ctypes_table_mirrors_header():
    from vamp_amd import _evid_lib
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(_evid_lib.SIGNATURES)
    assert len(protos["vamp_evid_run"][1]) == 33 and protos["vamp_evid_run"][1][18] == "uint64_t"
    for name, (ret, params) in protos.items():
        res, args = _evid_lib.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(args) == len(params), name
        for i, (ty, arg) in enumerate(zip(params, args)):
            assert arg is _CTYPES[ty] or arg == _CTYPES[ty], (name, i, ty, arg)


def test_other_libraries_untouched(evid_lib):
    """the evidence lives in its own library: the other headers, ctypes tables and libvamp_hip.so's exports do not name
    it, and the main ABI version is what it was"""
    import vamp_amd.build as vb
    from vamp_amd import _diag_lib, _lib, _post_lib
    assert not any("evid" in n for n in list(_lib.SIGNATURES) + list(_diag_lib.SIGNATURES) + list(_post_lib.SIGNATURES))
    main = open(os.path.join(ROOT, "include", "vamp_hip.h")).read()
    assert "vamp_evid" not in main and re.search(r"#define VAMP_ABI_VERSION 4\b", main)
    for h in ("vamp_diag.h", "vamp_post.h"):
        assert "vamp_evid" not in open(os.path.join(ROOT, "include", h)).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", vb.build(verbose=False)], text=True)
    exported = sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out)))
    assert exported == sorted(set(re.findall(r"\b(vamp_[a-z0-9_]+)\s*\(", _header_src("vamp_hip.h"))))
    src = open(os.path.join(ROOT, "vamp_amd", "csrc", "evidence.hip")).read()
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"../../include/vamp_evid.h", "draws.hpp", "lane_group.hpp", "side_call.hpp",
                                                               "voigt_math.hpp"}


def test_arguments_are_checked_before_any_device_call(evid_lib):
    """none of these reaches hipGetDeviceCount: on a machine without a GPU that call is what fails"""
    from vamp_amd import _evid_lib, evidence
    lib = _evid_lib.load()
    assert lib.vamp_evid_version() == 1
    x, flux, noise = ref.gauss_line_data(12, [(1.0, 5.0, 1.5)], 0.1, 8)
    base = {"x": x, "flux": flux, "noise": noise, "n_comp": 1, "mode": 0}

    def call(region=None, **kw):
        reg = dict(base, **(region or {}))
        args = dict(n_temps=4, walkers=8, steps=10, burn=2)
        args.update(kw)
        with pytest.raises(_evid_lib.EvidError) as e:
            evidence.log_evidence(reg, **args)
        assert "hip" not in str(e.value).lower()
        return str(e.value)

    assert "n_comp = 9" in call({"n_comp": 9})
    assert "n_comp = 0" in call({"n_comp": 0})
    assert "walkers = 7 must be even" in call(walkers=7)
    assert "walkers = 2 must be even" in call(walkers=2)
    assert "walkers = 258" in call(walkers=258)
    assert "n_temps = 1 is outside" in call(n_temps=1)
    assert "n_temps = 1 is outside" in call(betas=[1.0])
    assert "n_temps = 65 is outside" in call(n_temps=65)
    for bad in ([0.0, 0.5, 0.5, 1.0], [0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0, 0.7, 0.3, 1.0], [0.0, np.nan, 1.0]):
        assert "betas must increase strictly from 0 to 1" in call(betas=bad)
    wiggle = x.copy()
    wiggle[5] = wiggle[3]
    assert "strictly monotonic (pixel 5)" in call({"x": wiggle})
    flat = x.copy()
    flat[7] = flat[6]
    assert "strictly monotonic (pixel 7)" in call({"x": flat})
    assert "NBZ3" in call({"mode": 2})
    assert "mode must be" in call({"mode": 3})
    assert "noise must be positive" in call({"noise": np.zeros(12)})
    assert "not finite at pixel 2" in call({"flux": np.where(np.arange(12) == 2, np.nan, flux)})
    assert "empty prior range" in call({"bounds": (3.0, 3.0, 1.0, 1.0)})
    assert "one pixel needs bounds" in call({"x": x[:1], "flux": flux[:1], "noise": noise[:1]})
    assert "burn" in call(steps=10, burn=10)
    assert "swap_every" in call(swap_every=0)
    assert "stretch scale" in call(a=1.0)
    assert "region_id" in call({"region_id": -1})
    assert "region_id" in call({"region_id": 2 ** 31 - 1})
    bad_start = np.ones((8, 3))
    bad_start[2, 1] = np.inf
    assert "the start is not finite" in call(start=bad_start)
    with pytest.raises(ValueError):
        evidence.log_evidence(base, walkers=8, start=np.ones((8, 4)))
    with pytest.raises(ValueError):
        evidence.log_evidence(dict(base, noise=None))
    with pytest.raises(_evid_lib.EvidError, match="n_comp = 9"):
        evidence.lnlike(dict(base, n_comp=9), np.ones((2, 27)))
    with pytest.raises(_evid_lib.EvidError, match="NBZ3"):
        evidence.lnlike(dict(base, mode=2), np.ones((2, 3)))
    assert lib.vamp_evid_run(0, None, 0, *([None] * 9), 4, None, 8, 10, 2, 5, 1, 2.0, *([None] * 10), 0, None, None) == -1
    assert b"n_regions" in lib.vamp_evid_last_error()
    assert lib.vamp_evid_default_betas(5, None) == -1 and b"NULL" in lib.vamp_evid_last_error()


# ---- wiring, with the library call replaced by a fake ------------------------------------------------------------
@pytest.fixture
def fake_library(monkeypatch):
    from vamp_amd import evidence
    fake = ref.FakeLibrary()
    monkeypatch.setattr(evidence, "_run", fake)
    monkeypatch.setattr(evidence, "default_betas", ref.default_betas)
    return fake.calls


def _fake_fit(x, K, mode=0, chain=None):
    D = (4 if mode == 1 else 3) * K + 1
    return types.SimpleNamespace(_x=np.asarray(x), _flux=np.ones(len(x)), noise=None, _sample_sd=True, _n=K, _mode=mode, _chain_dev=chain,
                                 device=0, _ndim=D)


def test_fits_evidence_one_call_and_the_start(fake_library, monkeypatch):
    from vamp_amd import evidence
    x = np.arange(20.0)
    rng = np.random.default_rng(2)
    with_chain = _fake_fit(x, 2, chain=rng.random((5, 40, 7)))
    short_chain = _fake_fit(x, 1, chain=rng.random((5, 16, 4)))
    none = _fake_fit(x[:9], 1, mode=1)
    seen = {}
    real = evidence._run
    monkeypatch.setattr(evidence, "_run", lambda specs, betas, walkers, *a, **k: seen.update(specs=specs, starts=a[5]) or real(specs, betas, walkers, *a, **k))
    recs = evidence.fits_evidence([with_chain, short_chain, none], steps=40, burn=8, n_temps=6)
    assert fake_library == [3] and [f.evidence for f in (with_chain, short_chain, none)] == recs
    assert [s["region_id"] for s in seen["specs"]] == [0, 1, 2] and [s["n_comp"] for s in seen["specs"]] == [2, 1, 1]
    assert all(s["sample_sd"] and s["noise"] is None for s in seen["specs"]) and seen["specs"][2]["mode"] == 1
    np.testing.assert_array_equal(seen["starts"][0], with_chain._chain_dev[-1, :32])      # the last ensemble, as many walkers as asked
    assert seen["starts"][1] is None and seen["starts"][2] is None                        # too few walkers / no chain: prior draws
    assert recs[0].betas.size == 6 and recs[0].chain is None and math.isfinite(recs[0].lnZ) and recs[0].lnZ_se > 0
    assert evidence.fits_evidence([]) == [] and fake_library == [3]
    one = evidence.log_evidence({"x": x, "flux": np.ones(20), "noise": np.ones(20), "n_comp": 1}, return_chain=True)
    assert isinstance(one, evidence.Evidence) and one.chain.shape == (400, 32, 3) and fake_library == [3, 1]


def test_vpfit_log_evidence_is_kept_on_the_fit(fake_library):
    from vamp_amd.vpfits import VPfit
    fit = VPfit(seed=1)
    fit.__dict__.update(_fake_fit(np.arange(15.0), 2).__dict__)
    rec = fit.log_evidence(steps=30, burn=6)
    assert fit.evidence is rec and fake_library == [1] and rec.betas.size == 16


def test_region_fit_bic_calls_nothing_new_and_evidence_stops_at_two(fake_library, monkeypatch):
    from vamp_amd import vpregion
    x, flux, noise = ref.gauss_line_data(32, [(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)], 0.1, 4)
    fitted = []

    def fake_fit_n(self, n, iterations, thin, burn):
        fitted.append(n)
        bic = {1: 300.0, 2: 100.0, 3: 120.0}[n]
        return types.SimpleNamespace(bic_array=[bic] * 3, red_chi_array=[5.0] * 3, _n=n, _ctx=None)

    monkeypatch.setattr(vpregion.VPregion, "_fit_n", fake_fit_n)
    reg = vpregion.VPregion(1.0e3 + x, flux, noise, seed=5)
    assert reg.n == 1
    reg.region_fit(verbose=False)
    assert fake_library == [] and fitted == [1, 2, 3] and reg.n == 2 and not hasattr(reg, "evidences")       # today's path
    with pytest.raises(ValueError):
        reg.region_fit(verbose=False, criterion="aic")
    reg = vpregion.VPregion(1.0e3 + x, flux, noise, seed=5)
    del fitted[:]
    reg.region_fit(verbose=False, criterion="evidence", evidence_kw={"steps": 40, "burn": 8})
    assert fake_library == [1, 1, 1] and sorted(reg.evidences) == [1, 2, 3] and reg.n == 2      # the fake's ln Z peaks at two lines
    assert fitted == [2] and reg.fit._n == 2 and reg.fit.evidence is reg.evidences[2]          # the kept fit is find_bic's
    assert reg.evidences[2].lnZ - reg.evidences[1].lnZ > math.hypot(reg.evidences[1].lnZ_se, reg.evidences[2].lnZ_se)


def _fake_spectrum(tmp_path=None, VPspectrum=None):
    if VPspectrum is None:
        from vamp_amd.vpspectrum import VPspectrum
    spec = VPspectrum.__new__(VPspectrum)
    spec.wavelength_array, spec.flux_array, spec.region_pixels, spec.device = np.linspace(1210.0, 1220.0, 120), np.ones(120), [(10, 30), (50, 94)], 0
    spec.regions = []
    for (s, e), K in zip(spec.region_pixels, (1, 2)):
        x = np.arange(e - s) - 0.5 * (e - s - 1)
        spec.regions.append(types.SimpleNamespace(fit=_fake_fit(x, K), n=K, num_pixels=e - s, best_chi_squared=1.0))
    if tmp_path is not None:
        spec.output_filename = str(tmp_path / "spectrum_9_gauss_")
    return spec


def test_spectrum_evidences_layout(fake_library, tmp_path):
    from vamp_amd import h5min
    spec = _fake_spectrum(tmp_path)
    ev = spec.evidences(n_temps=5, steps=30, burn=6)
    assert fake_library == [2]
    assert set(ev) == {"lnZ", "lnZ_se", "lnZ_ti", "n_comp", "betas", "mean_lnL", "var_lnL", "move_accept", "swap_accept"}
    assert ev["lnZ"].shape == (2,) and ev["betas"].shape == (5,) and ev["mean_lnL"].shape == (2, 5) and ev["swap_accept"].shape == (2, 4)
    assert ev["n_comp"].tolist() == [1, 2] and ev["lnZ"][1] == spec.regions[1].fit.evidence.lnZ
    back = h5min.read(spec.write_evidence(ev))
    assert set(back) == set(ev)
    for k in ev:
        np.testing.assert_array_equal(back[k], ev[k])
    spec.regions[0].fit._n = 9                    # more lines than the library takes: left out, NaN rows
    ev = spec.evidences(n_temps=5, steps=30, burn=6)
    assert fake_library == [2, 1] and np.isnan(ev["lnZ"][0]) and np.isnan(ev["mean_lnL"][0]).all() and np.isfinite(ev["lnZ"][1])
    assert ev["n_comp"].tolist() == [9, 2] and ev["betas"].shape == (5,) and ev["swap_accept"].shape == (2, 4)


def test_do_vamp_evidence_is_opt_in(fake_library, monkeypatch, tmp_path, capsys):
    """the record field and the file only with --evidence; without it the record has exactly the fields it had"""
    from vamp_amd import diagnostics, do_vamp, h5min, vpspectrum
    made, real = [], vpspectrum.VPspectrum

    class Spec:
        def __new__(cls, *a, **kw):
            spec = _fake_spectrum(tmp_path, real)
            spec.chi_limit, spec.flux_model, spec.voigt, spec.dtype = 1.5, {"difficult_fit": False}, False, 0
            spec.fit_spectrum = lambda batched=False: {}
            made.append(spec)
            return spec

    monkeypatch.setattr(vpspectrum, "VPspectrum", Spec)
    monkeypatch.setattr(diagnostics, "fits_diagnostics", lambda fits, device=0: ([], 0))
    recs = []
    for flags in ([], ["--evidence"]):
        assert do_vamp.main([__file__, "1215.67", "--output_folder", str(tmp_path)] + flags) == 0
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("vamp_perf ")]
        recs.append(json.loads(line[0][len("vamp_perf "):]))
        assert os.path.exists(tmp_path / "spectrum_9_gauss_evidence.h5") == bool(flags)
    assert set(recs[1]) - set(recs[0]) == {"evidence_seconds"} and set(recs[0]) <= set(recs[1])
    assert fake_library == [2] and recs[1]["evidence_seconds"] >= 0
    back = h5min.read(str(tmp_path / "spectrum_9_gauss_evidence.h5"))
    assert back["lnZ"].shape == (2,) and back["betas"].shape == (16,) and back["n_comp"].tolist() == [1, 2]
    assert json.load(open(str(tmp_path / "spectrum_9_gauss_perf.json"))) == recs[1]
