"""CPU tests of PSIS-LOO: the numpy restatement (tests/loo_ref.py) against the analytic leave-one-out density of a
normal-mean model and against itself in extended precision on every input of the GPU comparison, the tail-length
table and each edge rule of include/vamp_loo.h, the planted errors the GPU bars must catch, the libvamp_loo.so
boundary (build, exports, ctypes table, argument checks before any device call) and the Python wiring (mcmc.loo,
fits_loo's time step, VPspectrum.loo, do_vamp --loo, the ladder of VPregion) with the library call replaced by the
restatement."""
import ctypes as C
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

import loo_ref as ref
import posterior_ref as pref
import predictive_ref
from conftest import ROOT, load_golden
from oracle import vamp_oracle as vo


# ---- the restatement ---------------------------------------------------------------------------------------
def test_restatement_against_analytic_loo_of_a_normal_mean():
    """30 data y_i ~ N(mu, 1) with one outlier, 4000 independent draws of mu from the exact (flat-prior) posterior.  The
    leave-one-out predictive density of y_i is N(mean of the others, 1 / 29 + 1) in closed form.  The restatement is an
    importance-sampling estimate from independent draws, so its error is Monte Carlo error: with the raw ratios
    r = 1 / p(y_i | mu_s) the estimate is -log mean(r), whose standard error is sd(r) / (sqrt(S) mean(r)) (delta method).
    Bar: 4 of those per datum (30 data: a 4 sigma excursion of any has probability 2e-3; the seed is fixed).  Plain
    lppd, which does not leave the datum out, must miss the same bar by far on the outlier."""
    rng = np.random.default_rng(1)
    P, S = 30, 4000
    y = rng.normal(0.3, 1.0, P)
    y[0] = 3.5
    mu = rng.normal(y.mean(), 1.0 / np.sqrt(P), S)
    ll = -0.5 * (y[None, :] - mu[:, None]) ** 2 - 0.5 * np.log(2 * np.pi)
    got = ref.from_loglik(ll)
    others = (y.sum() - y) / (P - 1)
    var = 1.0 / (P - 1) + 1.0
    exact = -0.5 * (y - others) ** 2 / var - 0.5 * np.log(2 * np.pi * var)
    ratio = np.exp(-ll)
    se = ratio.std(axis=0, ddof=1) / (np.sqrt(S) * ratio.mean(axis=0))
    err = np.abs(got["elpd_loo_pix"] - exact)
    print("normal mean: worst |elpd_loo - exact| %.4g, worst error / standard error %.3g, worst |lppd - exact| %.3g, khat %.3g .. %.3g"
          % (err.max(), (err / se).max(), np.abs(got["lppd"] - exact).max(), got["khat"].min(), got["khat"].max()))
    assert np.all(err <= 4.0 * se), (err / se).max()
    assert abs(got["lppd"][0] - exact[0]) > 20.0 * se[0]
    assert got["n_high_k"] == 0 and np.all(got["p_loo_pix"] > 0)
    assert got["elpd_loo"] == pytest.approx(exact.sum(), abs=4.0 * np.sqrt((se ** 2).sum()) + 4.0 * se.max())


@pytest.mark.parametrize("case", ref.COLUMN_CASES, ids=lambda c: "S%d-%s-sd%d" % (c[1], c[2], c[3]))
def test_float64_restatement_against_extended_precision(case):
    """on every input of the GPU column-stage comparison: khat to 1e-12, elpd to 1e-13 relative.  The GPU bars (1e-10,
    1e-11) are more than two orders above this, which is what licenses them; and no khat lies within 1e-6 of 0.7, so
    n_high_k cannot flip on a rounding"""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    ll, want = ref.column_case(case)
    elpd_l, khat_l = ref.columns(ll, np.longdouble)
    k, fin = want["khat"], np.isfinite(want["khat"])
    assert np.array_equal(fin, np.isfinite(khat_l)) and np.isfinite(want["elpd_loo_pix"]).all()
    dk = float(np.max(np.abs(k[fin] - khat_l[fin]), initial=0.0))
    de = float(np.max(np.abs(want["elpd_loo_pix"] - elpd_l) / np.maximum(1.0, np.abs(elpd_l))))
    print("S %5d %s free_sd %d: M %3d khat %.3g .. %.3g, float64 against long double: khat %.2g, elpd relative %.2g"
          % (case[1], case[2], case[3], ref.tail_len(case[1]), np.min(k), np.max(k[fin], initial=-np.inf), dk, de))
    assert dk <= 1e-12 and de <= 1e-13
    assert not fin.any() or np.min(np.abs(k[fin] - ref.HIGH_KHAT)) > 1e-6
    assert fin.all() == (case[1] > 20)


def test_tail_length_table():
    assert [ref.tail_len(n) for n in (20, 21, 225, 231, 16384)] == [4, 5, 45, 46, 384]
    assert ref.tail_len(225) == -(-225 // 5) == 45 and ref.tail_len(230) == -(-230 // 5) == 46      # ceil(n / 5) up to n = 230 ...
    assert -(-231 // 5) == 47 and 46 * 46 >= 9 * 231 > 45 * 45 and ref.tail_len(232) == 46            # ... the root from n = 231
    for n in range(1, 3000):
        m3 = int(np.ceil(3 * np.sqrt(n) - 1e-9))
        assert ref.tail_len(n) == min(-(-n // 5), m3), n
    assert ref.tail_len(1) == 1 and ref.tail_len(0) == 0


# ---- each rule of the definitions -----------------------------------------------------------------------------
def test_no_samples_and_one_sample():
    got = ref.from_loglik(np.zeros((0, 3)))
    assert got["n_used"] == 0 and got["n_high_k"] == 0
    for k in ref.PIX + ref.GRP:
        assert np.isnan(got[k]).all(), k
    one = ref.from_loglik(np.array([[-1.5, -0.25]]))
    np.testing.assert_array_equal(one["elpd_loo_pix"], [-1.5, -0.25])       # the one weight is 1
    np.testing.assert_array_equal(one["lppd"], [-1.5, -0.25])
    assert np.isposinf(one["khat"]).all() and one["n_high_k"] == 2 and one["elpd_loo"] == -1.75 and np.all(one["p_loo_pix"] == 0)


def test_constant_column_and_zero_quartile():
    """n = 200: M = 40, q = 10"""
    rng = np.random.default_rng(2)
    ll = rng.normal(-1.0, 0.3, (200, 4))
    ll[:, 0] = -0.7                                            # every ratio equal
    ll[:, 1] = np.where(np.arange(200) < 190, -2.0, -0.5)      # 190 tied largest ratios: tail and cutoff are all that value
    order = np.argsort(ll[:, 2])                               # ascending l = descending ratio: the tail is order[:40]
    ll[order[30:41], 2] = ll[order[40], 2]                     # the tail's 10 smallest ratios tie with the cutoff: x_10 = 0
    assert ref.tail_len(200) == 40
    got = ref.from_loglik(ll)
    assert np.isposinf(got["khat"][:3]).all() and np.isfinite(got["khat"][3]) and np.isfinite(got["elpd_loo_pix"]).all()
    assert got["elpd_loo_pix"][0] == pytest.approx(-0.7, abs=1e-14) and got["p_loo_pix"][0] == pytest.approx(0.0, abs=1e-14)
    for p in (1, 2):                                           # raw weights: the harmonic mean of the likelihoods
        assert got["elpd_loo_pix"][p] == pytest.approx(-np.log(np.mean(np.exp(-ll[:, p]))), rel=1e-13)
    assert got["n_high_k"] == 3 + int(got["khat"][3] > 0.7)


def test_nan_and_infinite_entries():
    rng = np.random.default_rng(3)
    ll = rng.normal(-1.0, 0.3, (50, 4))
    ll[7, 1] = np.nan
    ll[9, 2] = -np.inf
    ll[11, 3] = np.inf
    got = ref.from_loglik(ll)
    for k in ("elpd_loo_pix", "p_loo_pix", "khat"):
        assert np.isfinite(got[k][0]) and np.isnan(got[k][1:]).all(), k
    assert np.isnan(got["lppd"][1]) and np.isfinite(got["lppd"][2]) and np.isnan(got["lppd"][3])       # vamp_pred.h's rule
    assert np.isnan(got["elpd_loo"]) and got["n_high_k"] == 0          # a NaN khat is not counted
    skipped = ref.from_loglik(ll, skip=np.isin(np.arange(50), (7, 9, 11)))
    assert np.isfinite(skipped["elpd_loo_pix"]).all() and (skipped["n_used"], skipped["n_bad"]) == (47, 3)
    np.testing.assert_array_equal(skipped["elpd_loo_pix"], ref.from_loglik(np.delete(ll, (7, 9, 11), axis=0))["elpd_loo_pix"])


def test_all_bad_ensemble_is_nan_not_an_error():
    g = load_golden("lnprob_cases.npz")
    name = "H1215_r0_K2_m0_sd0"
    chain = np.ones((3, 4, 6))
    chain[:, :, 2] = 0.0          # sigma <= 0 everywhere
    got = ref.pointwise(g[name + "_x"], g[name + "_flux"], g[name + "_noise"], chain, 2, vo.MODE_GAUSS3, False)
    assert got["n_used"] == 0 and got["n_bad"] == 12 and got["n_high_k"] == 0 and np.isnan(got["ll"]).all()
    for k in ref.PIX + ref.GRP:
        assert np.isnan(got[k]).all(), k


# ---- the planted errors the GPU comparison must see ----------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ref.COLUMN_CASES if c[1] == 129 or c[1] == 1025], ids=lambda c: "S%d-%s-sd%d" % (c[1], c[2], c[3]))
@pytest.mark.parametrize("which", ref.PLANTS + ("dropped 65th sample",))
def test_planted_errors_miss_the_bars_by_orders_of_magnitude(which, case):
    """on inputs of the GPU comparison each planted error is at least 1e3 bars away in a per-pixel value and in a group sum"""
    ll, want = ref.column_case(case)
    got = ref.from_loglik(np.delete(ll, 64, axis=0)) if which == "dropped 65th sample" else ref.from_loglik(ll, plant=which)
    b = ref.bars(want)
    with np.errstate(all="ignore"):
        pix = max(float(np.nanmax(np.where(np.isfinite(got[k]) & np.isfinite(want[k]), np.abs(got[k] - want[k]), np.inf) / b[k])) for k in ("elpd_loo_pix", "khat"))
    grp = abs(got["elpd_loo"] - want["elpd_loo"]) / b["elpd_loo"] if np.isfinite(got["elpd_loo"]) else np.inf
    print(which, "worst per-pixel error / bar %.3g, group error / bar %.3g" % (pix, grp))
    assert pix >= 1e3 and grp >= 1e3
    got["n_used"], got["n_bad"] = want["n_used"], want["n_bad"]
    with pytest.raises(AssertionError):
        ref.check(got, want)


# ---- the library boundary ----------------------------------------------------------------------------------
def _header_src(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_functions(stem="loo"):
    return sorted(set(re.findall(r"\b(vamp_%s[a-z0-9_]+)\s*\(" % ("" if stem == "hip" else stem + "_"), _header_src("vamp_%s.h" % stem))))


@pytest.fixture(scope="module")
def loo_lib():
    import vamp_amd.build as vb
    return vb.build_loo(verbose=False)


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out)))


def test_loo_library_builds_and_exports_the_header(loo_lib):
    assert os.path.exists(loo_lib)
    names = _header_functions()
    assert names == ["vamp_loo_from_loglik", "vamp_loo_last_error", "vamp_loo_pointwise", "vamp_loo_version"]
    assert _exports(loo_lib) == names


def test_build_makes_six_libraries_and_leaves_the_other_five_alone():
    import vamp_amd.build as vb
    assert vb.build(verbose=False).endswith("libvamp_hip.so")
    for stem in ("hip", "diag", "post", "evid", "pred", "loo"):
        path = os.path.join(ROOT, "vamp_amd", "libvamp_%s.so" % stem)
        assert os.path.exists(path), stem
        assert _exports(path) == _header_functions(stem), stem           # nm -D: what each header declares, nothing of another
    csrc = lambda f: os.path.join(vb.HERE, "csrc", f)
    assert set(vb.LOO_DEPS) == {vb.LOO_SRC, csrc("voigt_math.hpp"), csrc("side_call.hpp"), csrc("lane_group.hpp"), csrc("chain_groups.hpp"),
                                csrc("pointwise_ll.hpp"), os.path.join(vb.HERE, "..", "include", "vamp_loo.h")}
    assert vb.LOO_SRC == csrc("loo.hip") and vb.LOO_OUT.endswith("libvamp_loo.so")
    assert vb.LOO_FLAGS == vb.PRED_FLAGS == vb.SIDE_FLAGS and "-fvisibility=hidden" in vb.LOO_FLAGS
    includes = set(re.findall(r'#include "([^"]+)"', open(vb.LOO_SRC).read()))
    assert includes == {"../../include/vamp_loo.h", "chain_groups.hpp", "lane_group.hpp", "pointwise_ll.hpp", "side_call.hpp", "voigt_math.hpp"}
    for name in ("vamp_hip.h", "vamp_diag.h", "vamp_post.h", "vamp_evid.h", "vamp_pred.h"):
        assert "vamp_loo" not in open(os.path.join(ROOT, "include", name)).read()
    assert "vamp_loo" not in open(csrc("predictive.hip")).read()
    src = open(os.path.join(ROOT, "include", "vamp_loo.h")).read()
    assert re.search(r"#define VAMP_LOO_ABI_VERSION 1\b", src) and re.search(r"#define VAMP_LOO_MAX_SAMPLES 16384\b", src)
    assert re.search(r"#define VAMP_LOO_MAX_COMPONENTS 32\b", src)


def test_design_carries_the_header_s_definitions_word_for_word():
    """the block from "Definitions." to "Everything is fp64." of the header, without the comment's " * ", is in DESIGN.md"""
    src = open(os.path.join(ROOT, "include", "vamp_loo.h")).read()
    block = src[src.index(" * Definitions.\n"):src.index(" * Everything is fp64.")]
    text = "".join(line[3:] if line.startswith(" * ") else line for line in block.splitlines(keepends=True))
    assert len(text.splitlines()) > 25 and text in open(os.path.join(ROOT, "DESIGN.md")).read()


_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const char*": C.c_char_p,
           "const double* const*": C.POINTER(C.c_void_p), "double* const*": C.POINTER(C.c_void_p),
           "const uint8_t* const*": C.POINTER(C.c_void_p), "double*": C.POINTER(C.c_double),
           "const int64_t*": C.POINTER(C.c_int64), "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32)}


def _header_prototypes():
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(vamp_loo_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_src("vamp_loo.h")):
        types_ = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm in ("void", ""):
                continue
            types_.append(re.sub(r"\s*\*", "*", re.sub(r"\s*\b\w+$", "", prm)).replace("*const", "* const"))
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types_)
    return protos


def test_loo_ctypes_table_mirrors_header():
    from vamp_amd import _loo_lib
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(_loo_lib.SIGNATURES)
    pw, fl = protos["vamp_loo_pointwise"][1], protos["vamp_loo_from_loglik"][1]
    assert len(pw) == 27 and pw[12] == "const int64_t*" and pw[15] == "int64_t" and pw[26] == "double* const*"
    assert len(fl) == 19 and fl[3] == "const double* const*" and fl[7] == "const uint8_t* const*" and fl[8] == "int64_t"
    assert pw[16:26] == fl[9:19]                                   # the same outputs in the same order
    for name, (ret, params) in protos.items():
        res, args = _loo_lib.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(args) == len(params), name
        for i, (ty, arg) in enumerate(zip(params, args)):
            assert arg is _CTYPES[ty] or arg == _CTYPES[ty], (name, i, ty, arg)


def test_limits_are_the_predictive_library_s():
    from vamp_amd import loo, predictive
    assert loo.MAX_SAMPLES == predictive.MAX_SAMPLES == 16384 and loo.time_step is predictive.time_step and loo.HIGH_KHAT == 0.7


def test_arguments_are_checked_before_any_device_call(loo_lib):
    from vamp_amd import _loo_lib, loo
    lib = _loo_lib.load()
    assert lib.vamp_loo_version() == 1
    x = np.linspace(-3.0, 3.0, 7)
    y, nz = np.ones(7), np.full(7, 0.1)
    chain = np.ones((10, 4, 7))

    def call(n=10, W=4, K=2, mode=0, sd=0, ld=28, base=chain.ctypes.data, xs=x, flux=y, noise=nz, scratch=0):
        with pytest.raises(_loo_lib.LooError) as e:
            loo._call(0, [xs], [flux], [noise], [K], [mode], [sd], [base], False, [ld], [n], [W], scratch)
        return str(e.value)

    assert "noise must be NULL" in call(sd=1)
    assert "NULL noise" in call(noise=None)
    bad = y.copy()
    bad[2] = np.nan
    assert "flux is not finite at pixel 2" in call(flux=bad)
    for v in (0.0, -0.1, np.nan, np.inf):
        bad = nz.copy()
        bad[4] = v
        assert "noise is not finite and positive at pixel 4" in call(noise=bad)
    assert "exceeds 16384" in call(n=16385, W=1, ld=6)
    assert "exceeds 16384" in call(n=128, W=129, ld=129 * 6)
    assert "mode 2 (NBZ3) is not supported: pass the chain in the GAUSS3 (0) or VOIGT4 (1) layout" in call(mode=2)
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
    assert lib.vamp_loo_pointwise(0, None, 0, *([None] * 7), None, 0, *([None] * 3), 0, *([None] * 10), None) == -1
    assert b"vamp_loo_pointwise: n_groups" in lib.vamp_loo_last_error()

    ll = np.zeros((30, 5))

    def call2(ptr=ll.ctypes.data, S=30, P=5, skips=None, scratch=0, G=1):
        with pytest.raises(_loo_lib.LooError) as e:
            loo._call_loglik(0, [ptr] * G, [S] * G, [P] * G, skips, False, scratch)
        return str(e.value)

    assert "NULL log-likelihood matrix" in call2(ptr=0)
    assert "n_pix must be positive" in call2(P=0)
    assert "n_samples must be positive" in call2(S=0)
    assert "n_samples = 16385 exceeds 16384" in call2(S=16385)
    assert "skip must be 0 or 1 at sample 4" in call2(skips=[np.array([0, 1, 0, 0, 2] + [0] * 25, dtype=np.uint8)])
    assert "less than one column of the largest group (240 bytes)" in call2(scratch=239)
    assert "scratch_bytes must not be negative" in call2(scratch=-1)
    assert lib.vamp_loo_from_loglik(0, None, 0, None, 0, None, None, None, 0, *([None] * 10)) == -1
    assert b"vamp_loo_from_loglik: n_groups" in lib.vamp_loo_last_error()
    assert lib.vamp_loo_from_loglik(0, None, 1, None, 0, None, None, None, 0, *([None] * 10)) == -1
    assert b"NULL argument" in lib.vamp_loo_last_error()
    with pytest.raises(ValueError):
        loo.pointwise_loo(x, y, nz, np.zeros((4, 4)), 1, 0)
    with pytest.raises(ValueError):
        loo.pointwise_loo(x, y, None, np.zeros((4, 4, 3)), 1, 0)      # free sd: a Gaussian line has 4 parameters
    with pytest.raises(ValueError):
        loo.loo_from_loglik(np.zeros(5))
    with pytest.raises(ValueError):
        loo._call_loglik(0, [ll.ctypes.data], [30], [5], [np.zeros(29, dtype=np.uint8)])


def test_record_pairs_with_compare():
    from vamp_amd import loo, predictive
    rng = np.random.default_rng(4)
    mk = lambda e: loo.LooRecord(2, elpd_loo_pix=e, p_loo_pix=np.zeros(9), khat=np.zeros(9), lppd=e, elpd_loo=float(e.sum()), elpd_loo_se=1.0,
                                 p_loo=0.0, n_high_k=0, n_used=5, n_bad=0)
    a, b = mk(rng.normal(size=9)), mk(rng.normal(size=9))
    assert a.elpd is a.elpd_loo_pix and a.looic == -2.0 * a.elpd_loo and a.step == 2
    d = b.elpd_loo_pix - a.elpd_loo_pix
    diff, se = predictive.compare(a, b)
    assert diff == pytest.approx(d.sum(), rel=1e-14) and se == pytest.approx(np.sqrt(9 * d.var(ddof=1)), rel=1e-13)


# ---- wiring, with the library call replaced by the restatement ------------------------------------------------
@pytest.fixture
def fake_library(monkeypatch):
    from vamp_amd import loo
    calls = []
    monkeypatch.setattr(loo, "_loo_host", ref.fake_loo_host(calls))
    return calls


def _golden(name="H1215_r0_K2_m0_sd0"):
    g = load_golden("lnprob_cases.npz")
    return g[name + "_x"], g[name + "_flux"], g[name + "_noise"]


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


def test_loo_is_cached_and_leaves_waic_alone(fake_library, monkeypatch):
    from vamp_amd import predictive
    x, flux, noise = _golden()
    rng = np.random.default_rng(46)
    chain = _chain(rng, x, 2, 0, 9, 6, True)
    fit = _fake_fit(x, flux, None, chain, 2, 0)
    rec = fit.mcmc.loo()
    assert fake_library == [(1, [1])] and fit.mcmc.loo() is rec and fake_library == [(1, [1])]
    want = ref.pointwise(x, flux, None, chain, 2, 0, True)
    for k in ref.PIX:
        np.testing.assert_array_equal(getattr(rec, k), want[k])
    assert rec.elpd is rec.elpd_loo_pix and rec.elpd_loo == want["elpd_loo"] and rec.looic == -2.0 * want["elpd_loo"]
    assert (rec.elpd_loo_se, rec.p_loo, rec.n_high_k, rec.n_used, rec.n_bad, rec.step) == (want["elpd_loo_se"], want["p_loo"], want["n_high_k"], 54, 0, 1)
    waic_calls = []
    monkeypatch.setattr(predictive, "_pred_host", predictive_ref.fake_pred_host(waic_calls))
    assert fit.mcmc.waic().lppd.shape == x.shape and waic_calls == [(1, [1])] and fit.mcmc.loo() is rec       # two caches
    np.testing.assert_array_equal(fit.mcmc.waic().lppd, rec.lppd)
    known = _fake_fit(x, flux, noise, chain[:, :, :6].copy(), 2, 0)
    assert known.mcmc.loo().elpd_loo == ref.pointwise(x, flux, noise, chain[:, :, :6], 2, 0, False)["elpd_loo"]
    none = _fake_fit(x, flux, None, chain, 2, 0)
    none._chain_dev = None
    with pytest.raises(RuntimeError):
        none.mcmc.loo()


def test_fits_loo_one_call_and_the_time_step(fake_library):
    from vamp_amd import loo
    x, flux, noise = _golden()
    rng = np.random.default_rng(47)
    short = _fake_fit(x, flux, noise, _chain(rng, x, 1, 1, 5, 4, False), 1, 1)
    long_ = _fake_fit(x[:3], flux[:3], None, _chain(rng, x[:3], 1, 0, 700, 64, True), 1, 0)      # 44 800 samples: every third time
    none = types.SimpleNamespace(mcmc=None, _chain_dev=None)
    have, recs = loo.fits_loo([short, none, long_])
    assert fake_library == [(2, [1, 3])] and have == [short, long_]
    assert [r.step for r in recs] == [1, 3]
    assert recs[1].n_used + recs[1].n_bad == 234 * 64
    want = ref.pointwise(x[:3], flux[:3], None, long_._chain_dev[::3], 1, 0, True)
    np.testing.assert_array_equal(recs[1].elpd_loo_pix, want["elpd_loo_pix"])
    assert long_.mcmc.loo() is recs[1] and fake_library == [(2, [1, 3])]           # the one call filled each fit's cache


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


_SPECTRUM_KEYS = {"elpd_loo_pix", "p_loo_pix", "khat", "lppd", "elpd_loo", "elpd_loo_se", "p_loo", "looic", "n_high_k", "n_used", "n_bad",
                  "n_comp", "time_step"}


def test_spectrum_loo_layout(fake_library):
    rng = np.random.default_rng(48)
    spec = _fake_spectrum(rng)
    out = spec.loo()
    assert fake_library == [(2, [1, 1])]                           # one call over the kept fits
    assert set(out) == _SPECTRUM_KEYS
    outside = np.ones(120, bool)
    for j, (s, e) in enumerate(spec.region_pixels):
        outside[s:e] = False
        fit = spec.regions[j].fit
        want = ref.pointwise(fit._x, fit._flux, None, fit._chain_dev, fit._n, 0, True)
        for k in ref.PIX:
            assert out[k].shape == (120,)
            np.testing.assert_array_equal(out[k][s:e], want[k][::-1])      # flipped like _harvest
        assert out["elpd_loo"][j] == want["elpd_loo"] and out["looic"][j] == -2 * want["elpd_loo"]
        assert out["elpd_loo_se"][j] == want["elpd_loo_se"] and out["n_used"][j] == want["n_used"] and out["n_high_k"][j] == want["n_high_k"]
    for k in ref.PIX:
        assert np.isnan(out[k][outside]).all()
    assert list(out["n_comp"]) == [1, 2] and list(out["time_step"]) == [1, 1]
    spec.regions[1].fit._chain_dev = None
    with pytest.raises(RuntimeError):
        spec.loo()


def test_do_vamp_loo_is_opt_in(fake_library, monkeypatch, tmp_path, capsys):
    """the record field and the file only with --loo; without it the record has exactly the fields it had"""
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
    for flags in ([], ["--loo"]):
        assert do_vamp.main([__file__, "1215.67", "--output_folder", str(tmp_path)] + flags) == 0
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("vamp_perf ")]
        recs.append(json.loads(line[0][len("vamp_perf "):]))
        assert os.path.exists(tmp_path / "spectrum_9_gauss_loo.h5") == bool(flags)
        assert not os.path.exists(tmp_path / "spectrum_9_gauss_predictive.h5")
    assert set(recs[1]) - set(recs[0]) == {"loo_seconds"} and set(recs[0]) <= set(recs[1])
    assert fake_library == [(2, [1, 1])] and recs[1]["loo_seconds"] >= 0
    back = h5min.read(str(tmp_path / "spectrum_9_gauss_loo.h5"))
    want = made[1].loo()
    assert set(back) == set(want) == _SPECTRUM_KEYS
    for k in want:
        np.testing.assert_array_equal(back[k], want[k])
        assert back[k].dtype == want[k].dtype, k


# ---- the ladder, with planted records -------------------------------------------------------------------------
def _ladder_region(monkeypatch, planted, calls):
    """a VPregion whose ``_fit_n`` makes chain-carrying stand-ins; their records are the restatement's with ``planted``
    per-pixel elpd_loo"""
    from vamp_amd import loo
    from vamp_amd.vpregion import VPregion
    monkeypatch.setattr(loo, "_loo_host", ref.fake_loo_host(calls, planted))
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


def test_loo_ladder_adds_a_line_at_rise_above_se_and_stops_at_rise_below(monkeypatch):
    from vamp_amd import predictive
    wiggle = np.where(np.arange(20) % 2 == 0, 1.0, -0.9)          # sum 1.0, paired se 4.4
    elpd = {1: np.zeros(20), 2: np.full(20, 0.5) + 0.01 * np.arange(20), 3: np.full(20, 0.5) + 0.01 * np.arange(20) + wiggle}
    calls = []
    region, built, closed = _ladder_region(monkeypatch, lambda k: elpd[k], calls)
    region.region_fit(verbose=False, iterations=10, thin=1, burn=0, criterion='loo')
    rung = lambda n: [n, ("sampled from the MAP", n, 10, 0, 1), ("polished", n)]      # the WAIC ladder's rungs
    assert built == rung(1) + rung(2) + rung(3) and region.n == 2 and region.fit._n == 2
    assert closed == [1, 3]                                        # the dropped fits are released, the kept one is not
    assert sorted(region.loo) == [1, 2, 3] and region.fit.loo is region.loo[2] and not hasattr(region, "predictive")
    assert [c[0] for c in calls] == [1, 1, 1]                      # one library call per rung
    np.testing.assert_array_equal(region.loo[2].elpd_loo_pix, elpd[2])
    up, se_up = predictive.compare(region.loo[1], region.loo[2])
    flat_, se_flat = predictive.compare(region.loo[2], region.loo[3])
    assert up > se_up and up == pytest.approx(11.9) and flat_ == pytest.approx(1.0) and 4.0 < se_flat < 5.0 and not flat_ > se_flat
    # a rise inside the standard error at the first rung: the first fit is kept
    first = {1: np.zeros(20), 2: wiggle}
    region, built, closed = _ladder_region(monkeypatch, lambda k: first[k], [])
    region.region_fit(verbose=False, criterion='loo')
    assert region.n == 1 and region.fit._n == 1 and [b for b in built if isinstance(b, int)] == [1, 2] and closed == [2]
    assert region.fit.loo is region.loo[1]


def test_other_ladders_make_no_loo_call_and_the_error_names_every_criterion(monkeypatch):
    calls = []
    region, built, closed = _ladder_region(monkeypatch, None, calls)
    region.region_fit(verbose=False, iterations=10, thin=1, burn=0)
    assert built == [1, 2] and region.n == 1 and calls == [] and not hasattr(region, "loo")
    with pytest.raises(ValueError, match="'bic', 'evidence' or 'waic' or 'loo'"):
        region.region_fit(verbose=False, criterion='aic')
