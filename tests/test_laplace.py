"""CPU tests of Laplace importance sampling (include/vamp_laplace.h, vamp_amd/laplace.py): the numpy restatement
(tests/laplace_ref.py) against itself and against known answers, every planted error caught by ``check`` at a named
stage, the library boundary (build, exports, ctypes table, argument checks before any device call) and the Python
wiring with the library call replaced by a fake.  The GPU tests are tests/test_gpu_laplace.py."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import evidence_ref
import laplace_ref as ref
import loo_ref
import sampler_stats
from conftest import ROOT
from oracle import vamp_oracle as vo


# ---- the restatement against itself -----------------------------------------------------------------------------
def test_draws_are_keyed_as_the_header_says():
    """the vectorised draws against the scalar Philox, counter {s, j, 5, region_id} and key (seed lo, seed hi), at the
    corners; an odd D drops the last z; another region id or seed gives other draws"""
    seed, rid, S, D = (7 << 32) | 12345, 9, 70, 5
    z, rho = ref.draws(S, D, rid, seed)
    assert z.shape == rho.shape == (S, D)
    for s, j in ((0, 0), (0, 2), (69, 1), (33, 2)):
        r = vo.philox4x32_10((s, j, ref.STREAM_NORMAL, rid), (seed & vo.MASK32, seed >> 32))
        u1, u2 = 1.0 - vo._u53(r[0], r[1]), vo._u53(r[2], r[3])
        rr = math.sqrt(-2.0 * math.log(u1))
        assert rho[s, 2 * j] == rr and z[s, 2 * j] == rr * np.cos(2.0 * np.pi * u2)
        if 2 * j + 1 < D:
            assert z[s, 2 * j + 1] == rr * np.sin(2.0 * np.pi * u2)
    assert np.array_equal(z[:, :4], ref.draws(S, 4, rid, seed)[0])
    assert not np.array_equal(z, ref.draws(S, D, rid + 1, seed)[0]) and not np.array_equal(z, ref.draws(S, D, rid, seed + 1)[0])
    assert np.array_equal(z[:20], ref.draws(20, D, rid, seed)[0])             # a sample does not depend on S


def test_restated_draws_are_standard_normal():
    """all S D restated z at S = 16 384 against the normal CDF, at the bar of the sampler statistics"""
    from scipy.special import ndtr
    z, _ = ref.draws(16384, 4, 3, ref.QUAD_SEED)
    lam = sampler_stats.ks_lambda(z, ndtr)
    print("sqrt(N) D_N of", z.size, "draws:", lam)
    assert lam <= sampler_stats.KS_BAR
    corr = np.corrcoef(z.T)
    assert np.max(np.abs(corr - np.eye(4))) * math.sqrt(z.shape[0]) <= sampler_stats.CORR_BAR
    assert np.all(np.isfinite(z)) and abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02


def test_weights_equal_the_loo_column_on_finite_ratios_and_take_minus_infinity():
    rng = np.random.default_rng(5)
    for n in (20, 21, 64, 400):
        r = -0.5 * rng.standard_normal(n) ** 2 * 3.0
        lw, khat, rmax = ref.psis_weights(r)
        elpd, khat_loo = loo_ref.psis_column(-r)
        assert khat == khat_loo and rmax == r.max() and np.all(lw <= 0)
        lwn = lw - (lw.max() + np.log(np.sum(np.exp(lw - lw.max()))))
        v = -r + lwn
        assert elpd == pytest.approx(v.max() + np.log(np.sum(np.exp(v - v.max()))), rel=1e-13)
    assert np.isinf(ref.psis_weights(r[:20])[1]) and np.isfinite(ref.psis_weights(r[:21])[1])      # M = 4 | 5
    # -inf entries: they stay -inf, they count in n (and so in M), and fewer than M + 1 finite values leave the raw ratios
    r = -0.5 * rng.standard_normal(100) ** 2 * 3.0
    M = loo_ref.tail_len(100)
    some = r.copy()
    some[::3] = -np.inf
    lw, khat, _ = ref.psis_weights(some)
    assert np.isfinite(khat) and np.array_equal(np.isneginf(lw), np.isneginf(some))
    few = np.full(100, -np.inf)
    few[:M] = r[:M]
    lw, khat, rmax = ref.psis_weights(few)
    assert np.isinf(khat) and np.array_equal(lw[:M], r[:M] - rmax)
    few[M] = r[M]
    assert np.isfinite(ref.psis_weights(few)[1])


def test_quadrature_case_meets_the_bound_of_the_gpu_test():
    """one Gaussian line on 24 pixels, ln Z = 8.227 by quadrature, S = 4096, inflate 1.5, the seed the GPU test uses: the form
    of the evidence test's bound.  The restatement: lnZ 8.2198, se 0.0129, khat -0.61, ess 2432"""
    o = ref.quadrature_run()
    print({k: o[k] for k in ("lnZ", "lnZ_se", "lnZ_psis", "khat", "ess", "n_out", "lnp_centre")}, o["mean"], o["sd"])
    assert o["status"] == 0 and o["lnZ_se"] <= 0.05
    assert abs(o["lnZ"] - ref.QUAD_LNZ) <= 4 * o["lnZ_se"] + 0.02
    assert abs(o["lnZ_psis"] - ref.QUAD_LNZ) <= 4 * o["lnZ_se"] + 0.02
    assert o["khat"] <= 0.7 and o["ess"] > 1000 and o["n_out"] == 0
    c = ref.quadrature_case()
    assert np.all(np.abs(o["mean"] - c["centre"]) < 0.2) and np.all(o["sd"] > 0)      # a 12-sigma line: the MAP is near the mean
    worst = ref.check(o, c, "the restatement against itself")
    assert set(worst) == set(ref.STAGES) and max(worst.values()) <= 1.0


def test_edge_rules():
    c = ref.voigt_edge_case()
    o = ref.run(c)
    assert o["status"] == 0 and 0.35 * c["S"] < o["n_out"] < 0.65 * c["S"] and o["n_out"] == int(np.isneginf(o["lnp"]).sum())
    assert np.array_equal(o["theta"][:, 2] < 0, np.isneginf(o["lnp"])) and np.isfinite(o["lnZ"])
    ref.check(o, c, "L on its bound")
    # the centre outside the prior: status 2; a factor that is no factor: status 1; a centre from which every draw is outside
    assert ref.run(dict(c, centre=np.array([1.2, 11.3, -0.1, 5.0])))["status"] == 2
    bad = c["chol"].copy()
    bad[2, 2] = 0.0
    o1 = ref.run(dict(c, chol=bad))
    assert o1["status"] == 1 and np.isnan(o1["lnZ"]) and np.all(np.isnan(o1["theta"]))
    upper = c["chol"].copy()
    upper[0, 3] = np.nan
    assert ref.run(dict(c, chol=upper))["status"] == 0                              # the upper triangle is not read
    assert ref.run(dict(c, centre=np.array([0.0, 11.3, 1.0, 5.0]), S=30))["status"] == 2       # A = 0: log(0 e^-0) = -inf
    # a centre ON a bound is inside (status 0); the draws beyond it are outside, by the sign of their z alone
    edge = dict(c, bounds=(0.0, 23.0, 11.5, 5.0), S=30, chol=np.diag([1e-6, 1e-6, 1e-6, 1e-6]))
    assert ref.run(edge)["status"] == 0
    far = ref.run(dict(edge, centre=np.array([1.2, 11.3, 1.0, 5.0])))                 # G on its upper bound
    assert far["status"] == 0 and 0 < far["n_out"] < 30 and np.array_equal(far["z"][:, 3] > 0, np.isneginf(far["lnp"]))


@pytest.mark.parametrize("plant, stage", list(zip(ref.PLANTS, ("lnq", "lnZ", "khat", "mean", "z"))))
def test_every_planted_error_fails_check_at_its_stage(plant, stage):
    """the restatement with one deliberate error, held to ``check`` like a library result: the assertion that fails names
    the stage the error is in.  The case has rejected draws (else dropping them changes nothing) and S = 400 (M = 60)"""
    c = ref.voigt_edge_case()
    ref.check(ref.run(c), c, "unplanted")
    with pytest.raises(AssertionError) as e:
        ref.check(ref.run(c, plant=plant), c, plant)
    print(plant, "->", e.value.args[0][:3])
    assert e.value.args[0][1] == stage


# ---- the library boundary ----------------------------------------------------------------------------------
def _header_src(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_functions():
    return sorted(set(re.findall(r"\b(vamp_laplace_[a-z0-9_]+)\s*\(", _header_src("vamp_laplace.h"))))


@pytest.fixture(scope="module")
def laplace_lib():
    import vamp_amd.build as vb
    return vb.build_laplace(verbose=False)


def test_laplace_library_builds_and_exports_the_header(laplace_lib):
    assert os.path.exists(laplace_lib)
    names = _header_functions()
    assert names == ["vamp_laplace_last_error", "vamp_laplace_points", "vamp_laplace_version"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", laplace_lib], text=True)
    assert sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out))) == names


def test_build_makes_nine_libraries():
    import vamp_amd.build as vb
    assert vb.build(verbose=False).endswith("libvamp_hip.so")
    for stem in ("hip", "diag", "post", "evid", "pred", "loo", "relabel", "fisher", "laplace"):
        assert os.path.exists(os.path.join(ROOT, "vamp_amd", f"libvamp_{stem}.so")), stem
    assert vb.LAPLACE_FLAGS is vb.SIDE_FLAGS and vb.LAPLACE_OUT.endswith("libvamp_laplace.so")
    csrc = lambda f: os.path.join(vb.HERE, "csrc", f)
    assert set(vb.LAPLACE_DEPS) == {vb.LAPLACE_SRC, csrc("voigt_math.hpp"), csrc("draws.hpp"), csrc("side_call.hpp"), csrc("lane_group.hpp"),
                                    os.path.join(vb.HERE, "..", "include", "vamp_laplace.h")}
    src = open(vb.LAPLACE_SRC).read()
    assert set(re.findall(r'#include "([^"]+)"', src)) == {"../../include/vamp_laplace.h", "draws.hpp", "lane_group.hpp", "side_call.hpp",
                                                               "voigt_math.hpp"}


_CTYPES = {"int": C.c_int, "uint64_t": C.c_uint64, "void*": C.c_void_p, "const char*": C.c_char_p,
           "const double* const*": C.POINTER(C.c_void_p), "double* const*": C.POINTER(C.c_void_p), "double*": C.POINTER(C.c_double),
           "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32)}


def _header_prototypes():
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(vamp_laplace_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_src("vamp_laplace.h")):
        types_ = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm in ("void", ""):
                continue
            types_.append(re.sub(r"\s*\*", "*", re.sub(r"\s*\b\w+$", "", prm)))
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types_)
    return protos


def test_laplace_ctypes_table_mirrors_header():
    from vamp_amd import _laplace_lib, laplace
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(_laplace_lib.SIGNATURES)
    assert len(protos["vamp_laplace_points"][1]) == 33 and protos["vamp_laplace_points"][1][15] == "uint64_t"
    for name, (ret, params) in protos.items():
        res, args = _laplace_lib.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(args) == len(params), name
        for i, (ty, arg) in enumerate(zip(params, args)):
            assert arg is _CTYPES[ty] or arg == _CTYPES[ty], (name, i, ty, arg)
    hdr = open(os.path.join(ROOT, "include", "vamp_laplace.h")).read()
    assert re.search(r"#define VAMP_LAPLACE_MAX_SAMPLES %d\b" % laplace.MAX_SAMPLES, hdr)
    assert re.search(r"#define VAMP_LAPLACE_MAX_COMPONENTS %d\b" % laplace.MAX_COMPONENTS, hdr)


def test_other_libraries_do_not_name_the_ninth():
    from vamp_amd import _evid_lib, _fisher_lib, _lib, _loo_lib
    assert not any("laplace" in n for m in (_lib, _evid_lib, _fisher_lib, _loo_lib) for n in m.SIGNATURES)
    for h in ("vamp_hip.h", "vamp_evid.h", "vamp_loo.h", "vamp_fisher.h"):
        assert "vamp_laplace_" not in open(os.path.join(ROOT, "include", h)).read()


def test_arguments_are_checked_before_any_device_call(laplace_lib):
    """none of these reaches hipGetDeviceCount: on a machine without a GPU that call is what fails"""
    from vamp_amd import _laplace_lib, laplace
    lib = _laplace_lib.load()
    assert lib.vamp_laplace_version() == 1
    x, flux, noise = evidence_ref.gauss_line_data(12, [(1.0, 5.0, 1.5)], 0.1, 8)
    base = dict(xs=[x], fluxes=[flux], noises=[noise], n_comp=[1], modes=[0], sample_sd=[0], bounds=[None], region_ids=[0],
                centres=[np.array([1.0, 5.0, 1.5])], chols=[0.1 * np.eye(3)], n_samples=64, seed=1)

    def call(**kw):
        args = dict(base, **kw)
        with pytest.raises(_laplace_lib.LaplaceError) as e:
            laplace._call(0, **args)
        assert "hip" not in str(e.value).lower()
        return str(e.value)

    assert "n_samples = 1 is outside 2 .. 16384" in call(n_samples=1)
    assert "n_samples = 16385 is outside" in call(n_samples=16385)
    assert "n_comp = 17" in call(n_comp=[17], centres=[np.ones(51)], chols=[np.eye(51)])
    assert "n_comp = 0" in call(n_comp=[0])
    assert "NBZ3" in call(modes=[2])
    assert "mode must be" in call(modes=[3])
    assert "sample_sd must be 0 or 1" in call(sample_sd=[2])
    assert "NULL noise" in call(noises=[None])
    assert "noise must be NULL" in call(sample_sd=[1], centres=[np.ones(4)], chols=[np.eye(4)])
    assert "noise must be positive" in call(noises=[np.zeros(12)])
    assert "not finite at pixel 2" in call(fluxes=[np.where(np.arange(12) == 2, np.nan, flux)])
    wiggle = x.copy()
    wiggle[5] = wiggle[3]
    assert "strictly monotonic (pixel 5)" in call(xs=[wiggle])
    assert "empty prior range" in call(bounds=[np.array([3.0, 3.0, 1.0, 1.0])])
    assert "one pixel needs bounds" in call(xs=[x[:1]], fluxes=[flux[:1]], noises=[noise[:1]])
    assert "region_id is negative" in call(region_ids=[-1])
    assert "group 1: NULL centre or chol" in call(**{k: v * 2 for k, v in base.items() if isinstance(v, list) and k != "centres"},
                                                  centres=[base["centres"][0], None])
    with pytest.raises(_laplace_lib.LaplaceError, match="samples_are_device"):
        _laplace_lib.check(_raw(lib, x, flux, noise, flag=2), lib)
    assert _raw(lib, x, flux, noise, groups=0) == -1 and b"n_groups" in lib.vamp_laplace_last_error()
    assert lib.vamp_laplace_points(0, None, 1, *([None] * 11), 64, 1, *([None] * 13), 0, None, None, None) == -1
    assert b"NULL argument" in lib.vamp_laplace_last_error()
    # what Python refuses itself
    c, v = np.array([1.0, 5.0, 1.5]), 0.01 * np.eye(3)
    with pytest.raises(ValueError, match="does not hold"):
        laplace.laplace_points(x, flux, noise, np.ones(4), v, 1, 0)
    with pytest.raises(ValueError, match="does not belong"):
        laplace.laplace_points(x, flux, noise, c, np.eye(4), 1, 0)
    with pytest.raises(ValueError, match="mode 2"):
        laplace.laplace_points(x, flux, noise, c, v, 1, 2)
    with pytest.raises(ValueError, match="n_comp"):
        laplace.laplace_points(x, flux, noise, np.ones(51), np.eye(51), 17, 0)
    with pytest.raises(ValueError, match="one abscissa"):
        laplace.laplace_points([x], [flux], [noise, noise], [c], [v], 1, 0)
    with pytest.raises(ValueError, match="inflate"):
        laplace.laplace_points(x, flux, noise, c, v, 1, 0, inflate=0.0)
    with pytest.raises(ValueError, match="unknown per-sample"):
        laplace.laplace_points(x, flux, noise, c, v, 1, 0, want=("weights",))
    with pytest.raises(ValueError, match="bounds must be"):
        laplace.laplace_points([x], [flux], [noise], [c], [v], 1, 0, bounds=[(0.0, 1.0)])
    assert laplace.laplace_points([], [], [], [], [], 1, 0) == [] and laplace.fits_laplace([]) == []


def _raw(lib, x, flux, noise, flag=0, groups=1):
    vp = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    i32 = lambda v: np.array([v], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    c, ch = np.array([1.0, 5.0, 1.5]), 0.1 * np.eye(3)
    return lib.vamp_laplace_points(0, None, groups, vp(x), vp(flux), vp(noise), i32(12), i32(1), i32(0), i32(0), None, i32(0), vp(c), vp(ch),
                                   64, 1, *([None] * 13), flag, None, None, None)


def test_proposal_factor():
    from vamp_amd import laplace
    cov = np.array([[4.0, 1.0], [1.0, 2.0]])
    c, logdet = laplace.proposal_factor(cov, inflate=1.5)
    assert np.allclose(c @ c.T, 2.25 * cov, rtol=1e-15) and np.array_equal(c, np.tril(c))
    assert logdet == pytest.approx(-math.log(np.linalg.det(cov)), rel=1e-14)
    for bad, st in ((np.array([[1.0, 2.0], [2.0, 1.0]]), 0), (cov, 1), (np.full((2, 2), np.nan), 0)):
        c, logdet = laplace.proposal_factor(bad, status=st)
        assert c.shape == (2, 2) and np.all(np.isnan(c)) and math.isnan(logdet)


# ---- wiring, with the library call replaced by a fake ------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    from vamp_amd import fisher, laplace
    lib = ref.FakeLibrary()
    monkeypatch.setattr(laplace, "_call", lib)
    lib.fisher_calls = []

    def fits_fisher(fits, with_prior=True, device=0, jac=False):
        lib.fisher_calls.append(len(fits))
        out = []
        for f in fits:
            D = f._theta_dev.size
            cov = np.diag(0.01 * (1.0 + np.arange(D))) + 0.001
            st = int(getattr(f, "_fisher_status", 0))
            rec = fisher.FisherRecord(np.zeros(D), np.linalg.inv(cov), cov if st == 0 else np.full((D, D), np.nan), np.sqrt(np.diag(cov)),
                                      -np.linalg.slogdet(cov)[1], 1.0, st)
            out.append(rec.to_units(f._scale, names=f._names))
        return out

    monkeypatch.setattr(fisher, "fits_fisher", fits_fisher)
    return lib


def _fake_fit(x, K, mode=0, real=False):
    from vamp_amd.vpfits import VPfit
    q = 4 if mode == 1 else 3
    D = q * K + 1
    dnu, mid = 3.0e9, 2.4e15
    scale = np.array(([1.0] + [dnu] * (q - 1)) * K + [1.0])
    shift = np.array(([0.0, mid] + [0.0] * (q - 2)) * K + [0.0])
    fields = dict(_x=np.asarray(x, dtype=np.float64), _flux=np.ones(len(x)), noise=None, _sample_sd=True, _n=K, _mode=mode, _q=q, device=0,
                  _ndim=D, _theta_dev=np.linspace(0.5, 1.5, D), _scale=scale, _shift=shift, _names=["p%d" % i for i in range(D)],
                  _laplace=None, _fisher=None)
    fit = VPfit(seed=1)
    fit.__dict__.update(fields)
    return fit


def test_fits_laplace_one_call_each_and_the_units(fake):
    from vamp_amd import laplace
    x = np.arange(20.0)
    fits = [_fake_fit(x, 2), _fake_fit(x[:9], 1, mode=1), _fake_fit(x, 1)]
    fits[2]._fisher_status = 1
    recs = laplace.fits_laplace(fits, n_samples=256, inflate=2.0, seed=5)
    assert fake.calls == [3] and fake.fisher_calls == [3]
    seen = fake.seen[0]
    assert seen["region_ids"] == [0, 1, 2] and seen["bounds"] == [None] * 3 and seen["n_samples"] == 256 and seen["seed"] == 5
    assert all(n is None for n in seen["noises"])
    for f, r, c, ch in zip(fits, recs, seen["centres"], seen["chols"]):
        D = f._theta_dev.size
        assert np.array_equal(c, f._theta_dev) and r.names == f._names and r.n_samples == 256 and r.inflate == 2.0
        assert f.laplace(n_samples=256, inflate=2.0, seed=5) is r                  # the cache is filled
        if getattr(f, "_fisher_status", 0):
            assert np.all(np.isnan(ch)) and r.status == 1 and np.isnan(r.lnZ) and np.isnan(r.lnZ_laplace) and not r.ok
            continue
        cov_dev = np.diag(0.01 * (1.0 + np.arange(D))) + 0.001
        assert np.allclose(ch @ ch.T, 4.0 * cov_dev, rtol=1e-12) and np.array_equal(ch, np.tril(ch))       # device units, inflated
        # the fake answers mean = centre + 0.01, cov = C C^T in device units: the record has them in the caller's
        assert np.allclose(r.mean, (f._theta_dev + 0.01) * f._scale + f._shift, rtol=1e-15)
        assert np.allclose(r.cov, 4.0 * cov_dev * np.outer(f._scale, f._scale), rtol=1e-12)
        assert np.allclose(r.sd, 2.0 * np.sqrt(np.diag(cov_dev)) * f._scale, rtol=1e-12)
        assert r.lnZ_laplace == pytest.approx(3.0 + 0.5 * D * math.log(2 * math.pi) + 0.5 * np.linalg.slogdet(cov_dev)[1], rel=1e-12)
        assert r.status == 0 and r.ok and r.lnZ == -5.0 * abs(f._n - 2)
    assert fake.calls == [3]
    # another argument, or a moved point: the cache does not answer
    assert fits[0].laplace(n_samples=128) is not recs[0] and fake.calls == [3, 1]
    again = fits[0].laplace(n_samples=128)
    fits[0]._theta_dev = fits[0]._theta_dev * 1.01
    assert fits[0].laplace(n_samples=128) is not again and fake.calls == [3, 1, 1]
    one = laplace.laplace_points(x, np.ones(20), np.ones(20), np.array([1.0, 5.0, 2.0]), 0.01 * np.eye(3), 1, 0, want=("theta", "lw"))
    assert isinstance(one, laplace.LaplaceRecord) and one.theta.shape == (4096, 3) and one.lw.shape == (4096,) and one.z is None
    with pytest.raises(ValueError, match="scales"):
        one.to_units(np.ones(4))


def _fake_spectrum(tmp_path=None, VPspectrum=None):
    if VPspectrum is None:
        from vamp_amd.vpspectrum import VPspectrum
    spec = VPspectrum.__new__(VPspectrum)
    spec.wavelength_array, spec.flux_array, spec.region_pixels, spec.device = np.linspace(1210.0, 1220.0, 120), np.ones(120), [(10, 30), (50, 94)], 0
    spec.regions = []
    for (s, e), K, mode in zip(spec.region_pixels, (1, 2), (0, 1)):
        x = np.arange(e - s) - 0.5 * (e - s - 1)
        spec.regions.append(types.SimpleNamespace(fit=_fake_fit(x, K, mode), n=K, num_pixels=e - s, best_chi_squared=1.0))
    if tmp_path is not None:
        spec.output_filename = str(tmp_path / "spectrum_9_gauss_")
    return spec


def test_spectrum_laplace_layout(fake, tmp_path):
    from vamp_amd import h5min
    spec = _fake_spectrum(tmp_path)
    lap = spec.laplace(n_samples=128)
    assert fake.calls == [2] and fake.fisher_calls == [2]
    assert set(lap) == {"lnZ", "lnZ_se", "lnZ_psis", "lnZ_laplace", "khat", "ess", "n_out", "status", "trusted", "n_comp", "mean", "sd",
                        "line_region"}
    assert lap["lnZ"].shape == (2,) and lap["mean"].shape == (3, 4) and lap["line_region"].tolist() == [0, 1, 1]
    assert np.isnan(lap["mean"][0, 3]) and np.all(np.isfinite(lap["mean"][1:])) and lap["trusted"].tolist() == [1, 1]
    f1 = spec.regions[1].fit
    assert np.array_equal(lap["mean"][2], f1.laplace(n_samples=128).mean[4:8]) and lap["n_comp"].tolist() == [1, 2]
    back = h5min.read(spec.write_laplace(lap))
    assert set(back) == set(lap)
    for k in lap:
        np.testing.assert_array_equal(back[k], lap[k])
    spec.regions[0].fit._n = 17                   # more lines than the library takes: left out, NaN rows
    lap = spec.laplace(n_samples=128)
    assert fake.calls == [2, 1] and np.isnan(lap["lnZ"][0]) and lap["status"].tolist() == [-1, 0] and lap["trusted"].tolist() == [0, 1]
    assert lap["mean"].shape == (19, 4) and np.all(np.isnan(lap["mean"][:17]))


def test_do_vamp_laplace_is_opt_in(fake, monkeypatch, tmp_path, capsys):
    """the record field and the file only with --laplace; without it the record has exactly the fields it had"""
    from vamp_amd import diagnostics, do_vamp, h5min, vpspectrum
    real = vpspectrum.VPspectrum

    class Spec:
        def __new__(cls, *a, **kw):
            spec = _fake_spectrum(tmp_path, real)
            spec.chi_limit, spec.flux_model, spec.voigt, spec.dtype = 1.5, {"difficult_fit": False}, False, 0
            spec.fit_spectrum = lambda batched=False: {}
            return spec

    monkeypatch.setattr(vpspectrum, "VPspectrum", Spec)
    monkeypatch.setattr(diagnostics, "fits_diagnostics", lambda fits, device=0: ([], 0))
    recs = []
    for flags in ([], ["--laplace"]):
        assert do_vamp.main([__file__, "1215.67", "--output_folder", str(tmp_path)] + flags) == 0
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("vamp_perf ")]
        recs.append(json.loads(line[0][len("vamp_perf "):]))
        assert os.path.exists(tmp_path / "spectrum_9_gauss_laplace.h5") == bool(flags)
    assert set(recs[1]) - set(recs[0]) == {"laplace_seconds"} and set(recs[0]) <= set(recs[1])
    assert fake.calls == [2] and recs[1]["laplace_seconds"] >= 0
    back = h5min.read(str(tmp_path / "spectrum_9_gauss_laplace.h5"))
    assert back["lnZ"].shape == (2,) and back["n_comp"].tolist() == [1, 2] and back["sd"].shape == (3, 4)
    assert json.load(open(str(tmp_path / "spectrum_9_gauss_perf.json"))) == recs[1]


def test_region_fit_laplace_ladder_and_its_stop(fake, monkeypatch):
    from vamp_amd import vpregion
    x, flux, noise = evidence_ref.gauss_line_data(32, [(1.2, 9.0, 2.0), (0.9, 22.0, 2.5)], 0.1, 4)
    fitted, released = [], []

    def fake_fit_n(self, n, iterations, thin, burn):
        fitted.append(n)
        fit = _fake_fit(np.arange(32.0), n)
        fit.bic_array, fit.red_chi_array = [{1: 300.0, 2: 100.0, 3: 120.0}.get(n, 150.0)] * 3, [5.0] * 3
        return fit

    monkeypatch.setattr(vpregion.VPregion, "_fit_n", fake_fit_n)
    monkeypatch.setattr(vpregion.VPregion, "_release", staticmethod(lambda fit: released.append(fit._n)))
    reg = vpregion.VPregion(1.0e3 + x, flux, noise, seed=5)
    assert reg.n == 1
    reg.region_fit(verbose=False)                                                  # the default is today's path
    assert fake.calls == [] and fitted == [1, 2, 3] and reg.n == 2 and not hasattr(reg, "laplaces")
    with pytest.raises(ValueError):
        reg.region_fit(verbose=False, criterion="aic")
    # the fake's ln Z peaks at two lines (0.01 standard error each)
    reg = vpregion.VPregion(1.0e3 + x, flux, noise, seed=5)
    del fitted[:], released[:]
    reg.region_fit(verbose=False, criterion="laplace", evidence_kw={"n_samples": 64})
    assert fitted == [1, 2, 3] and fake.calls == [1, 1, 1] and sorted(reg.laplaces) == [1, 2, 3] and reg.n == 2 and reg.fit._n == 2
    assert released == [1, 3] and reg.laplace_stop is None and reg.fit.laplace(n_samples=64) is reg.laplaces[2]
    assert reg.laplaces[2].lnZ - reg.laplaces[1].lnZ > math.hypot(0.01, 0.01) and fake.seen[0]["n_samples"] == 64
    # khat above 0.7 at two lines: the ladder stops there and says so, although ln Z would have risen
    fake.khat_of = lambda k: 0.9 if k == 2 else 0.3
    reg = vpregion.VPregion(1.0e3 + x, flux, noise, seed=5)
    del fitted[:], released[:]
    out = []
    monkeypatch.setattr("builtins.print", lambda *a, **k: out.append(" ".join(str(v) for v in a)))
    reg.region_fit(verbose=True, criterion="laplace")
    monkeypatch.undo()
    assert fitted == [1, 2] and reg.n == 1 and reg.fit._n == 1 and released == [2]
    assert reg.laplace_stop == (2, "khat 0.90 above 0.7") and any("not to be trusted (khat 0.90 above 0.7)" in ln for ln in out)
