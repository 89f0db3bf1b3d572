"""CPU tests of the chain diagnostics: the numpy restatement (tests/chain_diag_ref.py) against known
answers, the libvamp_diag.so boundary (build, exports, ctypes table, argument checks), and the wiring of
``mcmc.diagnostics()`` and do_vamp's perf record with the library call replaced by the restatement."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import chain_diag_ref as ref
from conftest import ROOT


def test_ar1_tau_matches_theory():
    rng = np.random.default_rng(11)
    for rho in (0.3, 0.6, 0.8):
        tau, n_eff, r_hat, window, reliable = ref.diagnostics(ref.ar1(rng, 4000, 64, 2, rho))
        want = (1 + rho) / (1 - rho)
        assert np.all(np.abs(tau / want - 1) < 0.10), (rho, tau)
        assert np.all(reliable) and np.all(window > 0)
        assert np.allclose(n_eff, 4000 * 64 / tau)
        assert np.all(np.abs(r_hat - 1) < 0.01)


def test_two_modes_give_large_r_hat():
    rng = np.random.default_rng(12)
    r_hat = ref.diagnostics(ref.two_modes(rng, 400, 32, 3))[2]
    assert np.all(r_hat > 1.5)


def test_stuck_walker():
    rng = np.random.default_rng(13)
    x = ref.ar1(rng, 300, 16, 2, 0.5)
    x[:, 5, 1] = 0.1                   # one walker never moves in parameter 1
    tau, n_eff, r_hat, window, reliable = ref.diagnostics(x)
    assert np.isfinite(tau[0]) and tau[1] == np.inf and n_eff[1] == 0 and not reliable[1] and window[1] == -1
    assert np.isfinite(r_hat[1])
    x[:, :, 0] = 2.5                   # every walker stuck at one value: V = 0 and B = 0
    assert np.isnan(ref.diagnostics(x)[2][0])
    x[:, :8, 0] = -1.0                 # stuck at two values: V = 0, B > 0
    assert ref.diagnostics(x)[2][0] == np.inf


def test_values_that_are_not_finite():
    """a NaN or an infinity anywhere in a parameter's series: tau = n_eff = r_hat = NaN, window -1, not reliable, for that
    parameter alone; the rule comes before "stuck" (a series that is constant but for a NaN is not finite, not stuck)"""
    rng = np.random.default_rng(16)
    clean = ref.ar1(rng, 300, 16, 5, 0.5)
    x = clean.copy()
    x[100, 3, 0] = np.nan
    x[299, 15, 1] = np.inf
    x[:, 5, 2] = 0.1
    x[0, 5, 2] = np.nan                # constant but for a NaN
    x[:, 6, 3] = 0.1                   # stuck, and finite
    x[17, 2, 3] = -np.inf              # ... beside an infinity in another walker: not finite comes first
    tau, n_eff, r_hat, window, reliable = ref.diagnostics(x)
    for a in (tau, n_eff, r_hat):
        assert np.all(np.isnan(a[:4]))
    assert np.all(window[:4] == -1) and not reliable[:4].any()
    want = ref.diagnostics(clean)
    for got, w in zip((tau, n_eff, r_hat, window, reliable), want):
        assert got[4] == w[4]
    assert np.isfinite(tau[4]) and window[4] > 0 and reliable[4]


def test_collapsed_tau_of_a_very_short_chain_is_never_reliable():
    """tau_{N-1} = 0 identically: white noise of N = 5 puts the window where tau_m has collapsed below 0; that tau is
    reported, but n_eff is not negative and the result is not reliable"""
    x = np.random.default_rng(0).standard_normal((5, 34, 400))
    tau, n_eff, r_hat, window, reliable = ref.diagnostics(x)
    assert np.median(tau) < 0.5 and (tau < 0).any() and not reliable.any()    # white noise has tau = 1
    assert np.all(np.isnan(n_eff[tau <= 0])) and np.all(n_eff[tau > 0] > 0)
    rng = np.random.default_rng(1)
    for N in (5, 8, 12, 30, 49):
        tau, n_eff, _, _, reliable = ref.diagnostics(rng.standard_normal((N, 34, 3)))
        assert not reliable.any() and not np.any(n_eff < 0), N


def test_short_chain_is_nan():
    x = np.random.default_rng(14).standard_normal((3, 8, 2))
    tau, n_eff, r_hat, window, reliable = ref.diagnostics(x)
    assert np.all(np.isnan(tau)) and np.all(np.isnan(n_eff)) and np.all(np.isnan(r_hat))
    assert np.all(window == -1) and not reliable.any()


def test_affine_invariance():
    rng = np.random.default_rng(15)
    x = ref.ar1(rng, 600, 32, 3, 0.7)
    a = ref.diagnostics(x)
    b = ref.diagnostics(x * np.array([3.0, -0.01, 250.0]) + np.array([1e3, 5.0, -7.0]))
    for u, v in zip(a[:3], b[:3]):
        assert np.allclose(u, v, rtol=1e-8)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


# ---- the library boundary ----------------------------------------------------------------------
def _header_functions():
    src = open(os.path.join(ROOT, "include", "vamp_diag.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vamp_diag_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def diag_lib():
    import vamp_amd.build as vb
    return vb.build_diag(verbose=False)


def test_diag_library_builds_and_exports_the_header(diag_lib):
    assert os.path.exists(diag_lib)
    names = _header_functions()
    assert names == ["vamp_diag_chains", "vamp_diag_last_error", "vamp_diag_version"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", diag_lib], text=True)
    assert sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out))) == names


# C type of include/vamp_diag.h -> the ctypes type that passes it
_CTYPES = {"int": C.c_int, "double": C.c_double, "void*": C.c_void_p, "const char*": C.c_char_p,
           "const double* const*": C.POINTER(C.c_void_p), "double*": C.POINTER(C.c_double),
           "const int64_t*": C.POINTER(C.c_int64), "const int32_t*": C.POINTER(C.c_int32),
           "int32_t*": C.POINTER(C.c_int32), "uint8_t*": C.POINTER(C.c_uint8)}


def _header_prototypes():
    """name -> (return type, [parameter types]) of every function include/vamp_diag.h declares"""
    src = open(os.path.join(ROOT, "include", "vamp_diag.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(vamp_diag_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types_ = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm in ("void", ""):
                continue
            ty = re.sub(r"\s*\b\w+$", "", prm)                 # drop the parameter name
            types_.append(re.sub(r"\s*\*", "*", ty))
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types_)
    return protos


def test_diag_ctypes_table_mirrors_header():
    """names, return types and every parameter's type, in order"""
    from vamp_amd import _diag_lib
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(_diag_lib.SIGNATURES)
    assert protos["vamp_diag_chains"][1][5] == "const int64_t*"          # the parser sees what the header says
    for name, (ret, params) in protos.items():
        res, args = _diag_lib.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(args) == len(params), name
        for i, (ty, arg) in enumerate(zip(params, args)):
            assert arg is _CTYPES[ty] or arg == _CTYPES[ty], (name, i, ty, arg)


def test_main_library_abi_untouched():
    """the diagnostics live in their own library: vamp_hip.h and its ctypes table do not name them"""
    from vamp_amd import _lib
    assert not any(n.startswith("vamp_diag") for n in _lib.SIGNATURES)
    assert "vamp_diag" not in open(os.path.join(ROOT, "include", "vamp_hip.h")).read()


def test_arguments_are_checked_before_any_device_call(diag_lib):
    from vamp_amd import _diag_lib, diagnostics
    lib = _diag_lib.load()
    assert lib.vamp_diag_version() == 1
    x = np.zeros((10, 4, 2))

    def call(n=10, W=4, D=2, ld=8, c=5.0, base=x.ctypes.data, groups=1):
        with pytest.raises(_diag_lib.DiagError) as e:
            diagnostics._call(0, [base] * max(groups, 1) if groups > 0 else [base], False, [ld], [n], [W], [D], c)
        return str(e.value)

    assert "exceeds 8192" in call(n=8193)
    assert "positive" in call(W=0)
    assert "ld < walkers * ndim" in call(ld=7)
    assert "NULL base" in call(base=0)
    assert "c must be" in call(c=0.0)
    assert lib.vamp_diag_chains(0, None, 0, None, 0, None, None, None, None, 5.0, None, None, None, None, None) == -1
    assert b"n_groups" in lib.vamp_diag_last_error()
    with pytest.raises(ValueError):
        diagnostics.chain_diagnostics(np.zeros((4, 4)))


# ---- wiring, with the library call replaced by the restatement -------------------------------------------
@pytest.fixture
def fake_library(monkeypatch):
    from vamp_amd import diagnostics
    calls = []

    def host(arrays, c, device):
        calls.append(len(arrays))
        outs = [ref.diagnostics(a, c) for a in arrays]
        return tuple(np.concatenate([o[i] for o in outs]) for i in range(5))

    monkeypatch.setattr(diagnostics, "_diag_host", host)
    return calls


def _fake_fit(chain, names, derived=None, thin=1):
    from vamp_amd.vpfits import _EnsembleMCMC
    fit = types.SimpleNamespace(_chain_dev=chain, device=0)
    mc = _EnsembleMCMC(fit)
    mc._flat = chain.reshape(-1, chain.shape[2])
    mc._names, mc._derived, mc._thin = list(names), dict(derived or {}), thin
    fit.mcmc = mc
    return fit


def test_mcmc_diagnostics_wiring(fake_library):
    rng = np.random.default_rng(16)
    chain = ref.ar1(rng, 200, 16, 5, 0.6)
    names = ["xexp_0", "est_centroid_0", "est_L_0", "est_G_0", "sd"]
    fit = _fake_fit(chain, names, {"est_sigma_0": ("est_G_0", lambda g: g / 2.3548)}, thin=5)
    before = dict(fit.mcmc.stats()["xexp_0"])
    d = fit.mcmc.diagnostics()
    assert fake_library == [1]
    tau, n_eff, r_hat, window, reliable = ref.diagnostics(chain)
    assert sorted(d) == sorted(names + ["est_sigma_0"])
    for i, nm in enumerate(names):
        assert set(d[nm]) == {"autocorrelation time", "n_eff", "r_hat", "reliable"}
        assert d[nm]["autocorrelation time"] == pytest.approx(tau[i] * 5, rel=1e-12)
        assert d[nm]["n_eff"] == pytest.approx(n_eff[i], rel=1e-12) and d[nm]["r_hat"] == pytest.approx(r_hat[i], rel=1e-12)
        assert d[nm]["reliable"] == bool(reliable[i])
    assert d["est_sigma_0"] == d["est_G_0"]
    fit.mcmc.diagnostics()
    assert fake_library == [1]                          # computed once per fit
    assert fit.mcmc.stats()["xexp_0"] == before         # stats() is what it was
    assert set(fit.mcmc.stats()["xexp_0"]) == {"n", "standard deviation", "mean", "quantiles", "mc error"}


def test_perf_record_fields_one_call(fake_library):
    from vamp_amd import do_vamp
    rng = np.random.default_rng(17)
    fits = [_fake_fit(ref.ar1(rng, 120, 16, 4, 0.3), ["a", "b", "c", "sd"]),
            _fake_fit(ref.two_modes(rng, 120, 16, 4), ["a", "b", "c", "sd"]),
            _fake_fit(ref.ar1(rng, 120, 16, 7, 0.95), ["a", "b", "c", "d", "e", "f", "sd"])]
    regs = [types.SimpleNamespace(fit=f, best_chi_squared=1.0 + i, n=1, num_pixels=30) for i, f in enumerate(fits)]
    spec = types.SimpleNamespace(regions=regs, chi_limit=1.5, flux_model={"difficult_fit": False}, voigt=False, dtype=0, device=0)
    rec = do_vamp.perf_record(spec, "spectrum_1.h5", 2.5, False)
    assert fake_library == [3]                          # the whole spectrum in one call
    assert rec["seconds"] == 2.5 and rec["regions"] == 3
    per = [ref.diagnostics(f._chain_dev) for f in fits]
    assert rec["min_n_eff"] == pytest.approx(min(p[1].min() for p in per), rel=1e-12)
    assert rec["max_r_hat"] == pytest.approx(max(p[2].max() for p in per), rel=1e-12)
    assert rec["frac_regions_n_eff_below_50"] == pytest.approx(np.mean([p[1].min() < 50 for p in per]))
    assert rec["frac_regions_unreliable_tau"] == pytest.approx(np.mean([not p[4].all() for p in per]))
    assert rec["max_r_hat"] > 1.5 and rec["diagnostics_seconds"] >= 0
    assert all(f.mcmc._diag is not None for f in fits)  # each fit's cache is filled by the one call
    assert rec["diagnostics_regions_skipped"] == 0
    import json
    assert json.loads(json.dumps(rec)) == rec


def test_perf_record_survives_chains_too_long_to_diagnose(fake_library):
    """a run of --iterations 10000 --thin 1 keeps more samples than the library takes (8192): the perf record is still
    written, with the long fits left out of the diagnostics and counted"""
    from vamp_amd import do_vamp
    rng = np.random.default_rng(18)
    short = _fake_fit(ref.ar1(rng, 120, 8, 4, 0.3), ["a", "b", "c", "sd"])
    long_ = _fake_fit(rng.standard_normal((9000, 8, 4)), ["a", "b", "c", "sd"])
    regs = [types.SimpleNamespace(fit=f, best_chi_squared=1.2, n=1, num_pixels=30) for f in (short, long_)]
    spec = types.SimpleNamespace(regions=regs, chi_limit=1.5, flux_model={"difficult_fit": False}, voigt=False, dtype=0, device=0)
    rec = do_vamp.perf_record(spec, "spectrum_2.h5", 3.0, False)
    old = {"spectrum", "regions", "lines", "pixels_in_regions", "seconds", "batched", "sampler_seconds_last_fits",
           "median_reduced_chi2", "frac_regions_below_chi_limit", "difficult_fit", "voigt", "dtype"}
    assert old <= set(rec) and rec["regions"] == 2 and rec["seconds"] == 3.0
    assert fake_library == [1] and rec["diagnostics_regions_skipped"] == 1
    assert rec["min_n_eff"] == pytest.approx(ref.diagnostics(short._chain_dev)[1].min(), rel=1e-12)
    assert short.mcmc._diag is not None and long_.mcmc._diag is None
    spec.regions = regs[1:]                             # nothing left to diagnose: the fields are None, the record is there
    rec = do_vamp.perf_record(spec, "spectrum_2.h5", 3.0, False)
    assert fake_library == [1] and rec["diagnostics_regions_skipped"] == 1
    assert rec["min_n_eff"] is None and rec["max_r_hat"] is None and old <= set(rec)
