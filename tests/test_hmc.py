"""CPU tests of preconditioned HMC (include/vamp_hmc.h, vamp_amd/hmc.py): the numpy restatement (tests/hmc_ref.py) against
finite differences, against itself run backwards and at half the step, against the exact posterior of one line with
three broken moves beside it, every planted error caught by ``check`` at a named stage, the library boundary (build,
exports, ctypes table, argument checks before any device call) and the Python wiring with the library call replaced by
a fake.  The GPU tests are tests/test_gpu_hmc.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import evidence_ref
import hmc_ref as ref
import sampler_stats
from conftest import ROOT
from oracle import vamp_oracle as vo


# ---- 1. the gradient of vamp_fisher.h is the gradient of vamp_evid.h's ln p ---------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sd", [False, True])
def test_gradient_equals_central_differences_of_ln_p(mode, sd):
    """fisher_ref's grad (with_prior = 1) against central differences of evidence_ref's ln p at interior points.  The step
    is h_d = 1e-4 times the metric's scale of the parameter; the truncation of the difference at h is (fd(2h) - fd(h)) / 3
    to leading order (the h^2 argument), so the bar is |fd(2h) - fd(h)| -- three times that -- plus the rounding of ln p
    itself, 64 eps |ln p| / h."""
    c = ref.lines_case(40 if mode == 0 else 65, 2, mode, sd, 4, 1, 1)
    scale = ref.metric_scale(c)
    worst = 0.0
    for th in c["start"]:
        lnp, g = ref.value_and_grad(c, th)
        assert np.isfinite(lnp)
        for d in range(th.size):
            fd = []
            for h in (1e-4 * scale[d], 2e-4 * scale[d]):
                a, b = th.copy(), th.copy()
                a[d] += h
                b[d] -= h
                fd.append((ref.target(c, a) - ref.target(c, b)) / (a[d] - b[d]))
            bar = abs(fd[1] - fd[0]) + 64 * ref.EPS * abs(lnp) / (1e-4 * scale[d])
            worst = max(worst, abs(g[d] - fd[0]) / bar)
            assert abs(g[d] - fd[0]) <= bar, (mode, sd, d, g[d], fd, bar)
    print("mode", mode, "sd", sd, "worst |grad - fd| / bar", worst)


# ---- 2. the integrator alone ------------------------------------------------------------------------------------------
REVERSAL_AMPLIFICATION = 10.0


def reversal_bar(case, theta, p):
    """what 2 L leapfrog updates may leave of a trajectory run forwards and back: each update rounds theta at eps_m |theta|
    and p at eps_m |p| -- in units of the metric's scale eps_m max(|theta| / scale, |p|) -- a chain of D terms adds D + 2
    more, and the 2 L steps of a stable trajectory amplify an error by no more than REVERSAL_AMPLIFICATION"""
    size = max(float(np.max(np.abs(theta) / ref.metric_scale(case))), float(np.max(np.abs(p))), 1.0)
    return 2 * case["L"] * (theta.size + 4) * ref.EPS * size * REVERSAL_AMPLIFICATION


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sd", [False, True])
def test_trajectory_returns_to_its_start_with_the_momentum_negated(mode, sd):
    c = ref.lines_case(40 if mode == 0 else 65, 2, mode, sd, 4, 8, 1)
    D = c["start"].shape[1]
    z = ref.momentum_draws([0], range(4), D, 0, 5)[0][0]
    for th, p in zip(c["start"], z):
        lnp, g = ref.value_and_grad(c, th)
        there = ref.leapfrog(c, th, lnp, g, p, c["eps"])
        assert not there["wall"]
        back = ref.leapfrog(c, there["theta"], there["lnp"], there["g"], -there["p"], c["eps"])
        bar = reversal_bar(c, th, p)
        err = max(float(np.max(np.abs(back["theta"] - th) / ref.metric_scale(c))), float(np.max(np.abs(back["p"] + p))))
        print("mode", mode, "sd", sd, "reversal error", err, "bar", bar, "dH", there["dH"], back["dH"])
        assert err <= bar and abs(there["dH"] + back["dH"]) <= 1e-9 * max(1.0, abs(lnp))
        # a first momentum step of eps instead of eps / 2 is not reversible
        wrong = ref.leapfrog(c, th, lnp, g, p, c["eps"], plant="a full first momentum step")
        wrong_back = ref.leapfrog(c, wrong["theta"], wrong["lnp"], wrong["g"], -wrong["p"], c["eps"], plant="a full first momentum step")
        assert float(np.max(np.abs(wrong_back["theta"] - th) / ref.metric_scale(c))) > 1e6 * bar


def test_energy_error_is_second_order_in_the_step():
    """|dH| at (eps, L = 4) against (eps / 2, L = 8) -- the same trajectory time from the same start and momentum -- has a
    ratio in [3, 5]; eps = 0.1 puts the restatement at 3.9 .. 4.02 on all 24 trajectories.  A first-order integrator (the
    half steps left out: a full first momentum step) gives 2."""
    first_order = []
    for a, b in ref.ratio_cases():
        D = a["start"].shape[1]
        z = ref.momentum_draws([0], range(6), D, 0, 5)[0][0]
        for th, p in zip(a["start"], z):
            lnp, g = ref.value_and_grad(a, th)
            da, db = ref.leapfrog(a, th, lnp, g, p, a["eps"])["dH"], ref.leapfrog(b, th, lnp, g, p, b["eps"])["dH"]
            assert 3.0 <= abs(da) / abs(db) <= 5.0, (a["mode"], a["sample_sd"], da, db)
            assert 3.85 <= abs(da) / abs(db) <= 4.1                      # the cases were chosen for this
            wa = ref.leapfrog(a, th, lnp, g, p, a["eps"], plant="a full first momentum step")["dH"]
            wb = ref.leapfrog(b, th, lnp, g, p, b["eps"], plant="a full first momentum step")["dH"]
            first_order.append(abs(wa) / abs(wb))
    print("first-order ratios: median", np.median(first_order))
    assert 1.6 <= np.median(first_order) <= 2.4


# ---- 3. invariance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd", [False, True])
def test_honest_move_keeps_the_exact_posterior_and_three_broken_moves_do_not(sd):
    """N = 4096 chains start from exact draws of the one-line posterior (sampler_stats.gauss_line_posterior); after T = 60
    moves of L = 2 the marginals of the honest move pass ks_lambda < KS_BAR at an acceptance in 0.6 .. 0.8, and each broken
    move misses the bar at the same N, T, eps.  Measured (fixed noise, eps 1.32 | free sd, eps 0.95): honest acceptance 0.649
    | 0.628, worst ks 0.84 | 1.54; accept always 39.4 | 16.5; dH without the kinetic terms 3.57 | 8.67; H0 from the previous
    proposal 3.82 | 4.63.

    A wrong but reversible, volume-preserving integrator -- C for C^T in the momentum update, a misplaced half step --
    stays invariant under the accept test and passes this: those errors are for the integrator tests above and the GPU
    tests' stage checks to catch."""
    post, X0, chol, kw = ref.invariance_leg(sd)
    assert max(ref.ks_of(post, X0)) < sampler_stats.KS_BAR                      # the exact draws themselves
    lnp, g = ref.gauss_line_value_grad(post, X0[:4])                           # the vectorised target is the restatement's
    c = ref.make_case(post.x, post.flux, None if sd else post.noise_fixed, 1, 0, X0[:4], chol, 0.5, 1, 1, 1)
    for i in range(4):
        l2, g2 = ref.value_and_grad(c, X0[i])
        assert np.allclose(g[i], g2, rtol=1e-10, atol=1e-10) and abs((lnp[i] - lnp[0]) - (l2 - ref.value_and_grad(c, X0[0])[0])) < 1e-9
    figures = {}
    for broken in (None,) + ref.BROKEN:
        X, n_acc, n_wall = ref.vector_hmc(post, X0, chol, kw["eps"], kw["n_leap"], kw["n_steps"], np.random.default_rng(ref.INVARIANCE_SEED),
                                          broken=broken)
        figures[broken] = (float(n_acc.mean()) / kw["n_steps"], max(ref.ks_of(post, X)))
        print("sd", sd, broken or "honest", "acceptance %.3f worst ks %.2f walls %.4f" % (*figures[broken], float(n_wall.mean()) / kw["n_steps"]))
    assert 0.6 <= figures[None][0] <= 0.8 and figures[None][1] < sampler_stats.KS_BAR
    for broken in ref.BROKEN:
        assert figures[broken][1] > sampler_stats.KS_BAR, broken


def test_scalar_and_vector_restatements_walk_alike():
    """the scalar restatement (the GPU tests' yardstick) and the vectorised one make the same step from the same state,
    momentum and uniforms"""
    post, X0, chol, kw = ref.invariance_leg(False)
    c = ref.make_case(post.x, post.flux, post.noise_fixed, 1, 0, X0[:8], chol, 0.9, 3, 1, 1)
    z = ref.momentum_draws([0], range(8), 3, 0, 1)[0][0]

    class Fixed:                      # hands vector_hmc the momenta z and uniforms that accept nothing
        def standard_normal(self, shape):
            return z.copy()

        def random(self, n):
            return np.full(n, 0.5)

    lnp0, _ = ref.gauss_line_value_grad(post, X0[:8])
    X, n_acc, _ = ref.vector_hmc(post, X0[:8], chol, 0.9, 3, 1, Fixed(), broken="accept always")
    for i in range(8):
        lnp, g = ref.value_and_grad(c, X0[i])
        tr = ref.leapfrog(c, X0[i], lnp, g, z[i], 0.9)
        assert not tr["wall"] and np.allclose(X[i], tr["theta"], rtol=0, atol=1e-12)


# ---- 4. planted errors --------------------------------------------------------------------------------------------------
def _planted_case(plant):
    """rejections (else a stale g changes nothing), an even D for the dropped z, a thin grid to shift"""
    return ref.lines_case(40, 2, 0, plant != "the last z dropped at even D", 4, 1, 16, eps=1.5, thin=2, n_burn=3)


@pytest.mark.parametrize("plant, stage", list(zip(ref.PLANTS, ("prop", "prop", "mom", "prop", "chain"))))
def test_every_planted_error_fails_check_at_its_stage(plant, stage):
    c = _planted_case(plant)
    honest = ref.run(c)
    assert 0 < int(np.sum(honest["acc"] == 0)) < honest["acc"].size
    ref.check(honest, c, "unplanted")
    with pytest.raises(AssertionError) as e:
        ref.check(ref.run(c, plant=plant), c, plant)
    print(plant, "->", e.value.args[0][:4])
    assert e.value.args[0][1] == stage


def test_planted_errors_fail_at_eight_leaps_too():
    c = ref.lines_case(40, 2, 0, True, 2, 8, 6, eps=0.9)
    bars = ref.measured_bars(c)
    ref.check(ref.run(c), c, "unplanted", bars=bars)
    for plant in ("C for C^T", "a full first momentum step"):
        with pytest.raises(AssertionError) as e:
            ref.check(ref.run(c, plant=plant), c, plant, bars=bars)
        assert e.value.args[0][1] == "prop"


def test_restatement_edges():
    """the kept grid; a wall leaves the state bit for bit; statuses 1 and 2; a continued run; momenta given"""
    assert ref.kept_steps(7, 0, 3) == [0, 3, 6] and ref.kept_steps(5, 4, 2) == [4] and ref.kept_steps(6, 1, 2) == [1, 3, 5]
    from vamp_amd import hmc
    assert [hmc.n_keep_of(*a) for a in ((7, 0, 3), (5, 4, 2), (6, 1, 2), (1, 0, 1))] == [3, 1, 3, 1]
    w = ref.wall_case()
    o = ref.run(w)
    walls = o["acc"] == 2
    assert 0.3 * walls.size < walls.sum() < 0.8 * walls.size and np.all(np.isnan(o["dH"][walls])) and np.array_equal(o["n_wall"], walls.sum(axis=0))
    for c in range(4):
        for t in range(1, w["n_steps"]):
            if walls[t, c]:
                assert np.array_equal(o["chain"][t, c], o["chain"][t - 1, c]) and o["lnp"][t, c] == o["lnp"][t - 1, c]
    assert np.array_equal(walls, o["prop"][:, :, 2] < 0)                      # L_fwhm below 0, and nothing else, is the wall here
    ref.check(o, w, "walls")
    bad = w["chol"].copy()
    bad[2, 2] = 0.0
    o1 = ref.run(dict(w, chol=bad))
    assert o1["status"] == 1 and np.all(np.isnan(o1["chain"])) and np.all(o1["chain_status"] == 1)
    assert ref.run(dict(w, eps=0.0))["status"] == 1 and ref.run(dict(w, jitter=1.0))["status"] == 1
    start = w["start"].copy()
    start[1, 2] = -0.01
    w2 = dict(w, start=start)
    o2 = ref.run(w2)
    assert list(o2["chain_status"]) == [0, 2, 0, 0] and np.all(np.isnan(o2["chain"][:, 1])) and np.array_equal(o2["chain"][:, 0], o["chain"][:, 0])
    ref.check(o2, w2, "a bad start")
    # two calls of six steps are one of twelve
    first = ref.run(dict(w, n_steps=6))
    second = ref.run(dict(w, n_steps=6, step0=6, start=first["last"]))
    assert np.array_equal(np.concatenate([first["chain"], second["chain"]]), o["chain"])
    # the run's own momenta given back reproduce it; chain c alone through chain_id0
    again = ref.run(w, mom_in=o["mom"])
    assert all(np.array_equal(again[k], o[k], equal_nan=True) for k in ("chain", "prop", "dH", "acc"))
    ref.check(again, w, "momenta given", mom_in=o["mom"])
    alone = ref.run(dict(w, start=w["start"][2:3], chain_id0=2))
    assert np.array_equal(alone["chain"][:, 0], o["chain"][:, 2])


def test_draws_are_keyed_as_the_header_says():
    seed, rid = (7 << 32) | 12345, 9
    z, rho = ref.momentum_draws([3, 70], [0, 5, (1 << 26) - 1], 5, rid, seed)
    u, up = ref.accept_draws([3, 70], [0, 5, (1 << 26) - 1], rid, seed)
    key = (seed & vo.MASK32, seed >> 32)
    for ti, t in enumerate((3, 70)):
        for ci, c in enumerate((0, 5, (1 << 26) - 1)):
            for j in range(3):
                r = vo.philox4x32_10((t, c * 64 + j, 6, rid), key)
                u1, u2 = 1.0 - vo._u53(r[0], r[1]), vo._u53(r[2], r[3])
                rr = math.sqrt(-2.0 * math.log(u1))
                assert z[ti, ci, 2 * j] == rr * np.cos(2.0 * np.pi * u2)
                if 2 * j + 1 < 5:
                    assert z[ti, ci, 2 * j + 1] == rr * np.sin(2.0 * np.pi * u2)
            r = vo.philox4x32_10((t, c * 64 + 63, 7, rid), key)
            assert u[ti, ci] == 1.0 - vo._u53(r[0], r[1]) and up[ti, ci] == vo._u53(r[2], r[3])
    assert np.array_equal(z[:, :, :4], ref.momentum_draws([3, 70], [0, 5, (1 << 26) - 1], 4, rid, seed)[0])      # the last z of an odd D is dropped
    from scipy.special import ndtr
    zz = ref.momentum_draws(np.arange(64), np.arange(64), 4, 3, 1)[0]
    assert sampler_stats.ks_lambda(zz.ravel(), ndtr) <= sampler_stats.KS_BAR


def test_no_accept_decision_of_the_gpu_cases_is_too_close_to_compare():
    """the share of steps that ``check`` would leave out (|log u - dH| <= 1e-6) is zero in the restatement of every case the
    GPU tests run, and the decisions case has both outcomes"""
    cases = [ref.shape_case(n, L) for L in (1, 8) for n in ref.SHAPES] + [ref.wall_case(), ref.decisions_case()]
    for c in cases:
        o = ref.run(c)
        steps = c["step0"] + np.arange(c["n_steps"])
        u, _ = ref.accept_draws(steps, c["chain_id0"] + np.arange(len(c["start"])), c["region_id"], c["seed"])
        free = o["acc"] != 2
        assert np.all(np.abs(np.log(u[free]) - o["dH"][free]) > ref.DECISION_GAP)
    d = ref.run(ref.decisions_case())["acc"]
    assert 0.2 * d.size < np.sum(d == 0) < 0.8 * d.size and not np.any(d == 2)


# ---- 5. the library boundary ----------------------------------------------------------------------------------------
def _header_src():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vamp_hmc.h")).read(), flags=re.S)


def _header_functions():
    return sorted(set(re.findall(r"\b(vamp_hmc_[a-z0-9_]+)\s*\(", _header_src())))


@pytest.fixture(scope="module")
def hmc_lib():
    import vamp_amd.build as vb
    return vb.build_hmc(verbose=False)


def test_hmc_library_builds_and_exports_the_header(hmc_lib):
    assert os.path.exists(hmc_lib)
    names = _header_functions()
    assert names == ["vamp_hmc_chains", "vamp_hmc_last_error", "vamp_hmc_version"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", hmc_lib], text=True)
    assert sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out))) == names


def test_build_makes_ten_libraries():
    import vamp_amd.build as vb
    assert vb.build(verbose=False).endswith("libvamp_hip.so")
    for stem in ("hip", "diag", "post", "evid", "pred", "loo", "relabel", "fisher", "laplace", "hmc"):
        assert os.path.exists(os.path.join(ROOT, "vamp_amd", f"libvamp_{stem}.so")), stem
    assert vb.HMC_FLAGS is vb.SIDE_FLAGS and vb.HMC_OUT.endswith("libvamp_hmc.so")
    csrc = lambda f: os.path.join(vb.HERE, "csrc", f)
    deps = {"voigt_math.hpp", "voigt_grad.hpp", "draws.hpp", "side_call.hpp", "lane_group.hpp"}
    assert set(vb.HMC_DEPS) == {vb.HMC_SRC, os.path.join(vb.HERE, "..", "include", "vamp_hmc.h")} | {csrc(f) for f in deps}
    assert set(re.findall(r'#include "([^"]+)"', open(vb.HMC_SRC).read())) == {"../../include/vamp_hmc.h"} | deps


_CTYPES = {"int": C.c_int, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "void*": C.c_void_p, "const char*": C.c_char_p,
           "const double* const*": C.POINTER(C.c_void_p), "double* const*": C.POINTER(C.c_void_p), "int32_t* const*": C.POINTER(C.c_void_p),
           "double*": C.POINTER(C.c_double), "const double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32),
           "int32_t*": C.POINTER(C.c_int32)}


def _header_prototypes():
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(vamp_hmc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_src()):
        types_ = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm in ("void", ""):
                continue
            types_.append(re.sub(r"\s*\*", "*", re.sub(r"\s*\b\w+$", "", prm)))
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types_)
    return protos


def test_hmc_ctypes_table_mirrors_header():
    from vamp_amd import _hmc_lib, hmc
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(_hmc_lib.SIGNATURES)
    params = protos["vamp_hmc_chains"][1]
    assert len(params) == 41 and params[23] == "int64_t" and params[24] == "uint64_t"
    for name, (ret, params) in protos.items():
        res, args = _hmc_lib.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(args) == len(params), name
        for i, (ty, arg) in enumerate(zip(params, args)):
            assert arg is _CTYPES[ty] or arg == _CTYPES[ty], (name, i, ty, arg)
    hdr = open(os.path.join(ROOT, "include", "vamp_hmc.h")).read()
    assert re.search(r"#define VAMP_HMC_MAX_COMPONENTS %d\b" % hmc.MAX_COMPONENTS, hdr)
    assert re.search(r"#define VAMP_HMC_MAX_LEAP %d\b" % hmc.MAX_LEAP, hdr)
    assert re.search(r"#define VAMP_HMC_MAX_CHAIN_ID \(1 << 26\)", hdr) and hmc.MAX_CHAIN_ID == 1 << 26


def test_other_libraries_do_not_name_the_tenth():
    from vamp_amd import _fisher_lib, _laplace_lib, _lib
    assert not any("hmc" in n for m in (_lib, _fisher_lib, _laplace_lib) for n in m.SIGNATURES)
    for h in ("vamp_hip.h", "vamp_evid.h", "vamp_fisher.h", "vamp_laplace.h"):
        assert "vamp_hmc_" not in open(os.path.join(ROOT, "include", h)).read()


def test_arguments_are_checked_before_any_device_call(hmc_lib):
    """none of these reaches hipGetDeviceCount: on a machine without a GPU that call is what fails"""
    from vamp_amd import _hmc_lib, hmc
    lib = _hmc_lib.load()
    assert lib.vamp_hmc_version() == 1
    x, flux, noise = evidence_ref.gauss_line_data(12, [(1.0, 5.0, 1.5)], 0.1, 8)
    base = dict(xs=[x], fluxes=[flux], noises=[noise], n_comp=[1], modes=[0], sample_sd=[0], bounds=[None], region_ids=[0], n_chains=[2],
                chain_id0=[0], starts=[np.tile([1.0, 5.0, 1.5], (2, 1))], chols=[0.1 * np.eye(3)], eps=[0.5], jitter=[0.0], n_leap=4, n_steps=8)

    def call(**kw):
        args = dict(base, **kw)
        with pytest.raises(_hmc_lib.HmcError) as e:
            hmc._call(0, **args)
        assert "hip" not in str(e.value).lower()
        return str(e.value)

    assert "n_leap = 0 is outside 1 .. 64" in call(n_leap=0)
    assert "n_leap = 65 is outside" in call(n_leap=65)
    assert "n_steps must be positive" in call(n_steps=0)
    assert "n_burn = 8 is outside" in call(n_burn=8)
    assert "n_burn = -1 is outside" in call(n_burn=-1)
    assert "thin must be at least 1" in call(thin=0)
    assert "step0 + n_steps" in call(step0=(1 << 31) - 7)
    assert "step0 + n_steps" in call(step0=-1)
    assert "n_comp = 17" in call(n_comp=[17], starts=[np.ones((2, 51))], chols=[np.eye(51)])
    assert "n_comp = 0" in call(n_comp=[0])
    assert "NBZ3" in call(modes=[2])
    assert "mode must be" in call(modes=[3])
    assert "sample_sd must be 0 or 1" in call(sample_sd=[2])
    assert "NULL noise" in call(noises=[None])
    assert "noise must be NULL" in call(sample_sd=[1], starts=[np.ones((2, 4))], chols=[np.eye(4)])
    assert "noise must be positive" in call(noises=[np.zeros(12)])
    assert "not finite at pixel 2" in call(fluxes=[np.where(np.arange(12) == 2, np.nan, flux)])
    wiggle = x.copy()
    wiggle[5] = wiggle[3]
    assert "strictly monotonic (pixel 5)" in call(xs=[wiggle])
    assert "empty prior range" in call(bounds=[np.array([3.0, 3.0, 1.0, 1.0])])
    assert "one pixel needs bounds" in call(xs=[x[:1]], fluxes=[flux[:1]], noises=[noise[:1]])
    assert "region_id is negative" in call(region_ids=[-1])
    assert "chain identities" in call(chain_id0=[-1])
    assert "chain identities" in call(chain_id0=[(1 << 26) - 1])
    assert "group 1: NULL start or chol" in call(**{k: v * 2 for k, v in base.items() if isinstance(v, list) and k != "chols"},
                                                 chols=[base["chols"][0], None])
    assert "kept states" in call(n_chains=[1 << 20], chain_id0=[0], starts=[np.ones((1 << 20, 3))], n_steps=1 << 10)
    assert "in a trace" in call(n_chains=[1 << 20], starts=[np.ones((1 << 20, 3))], n_steps=1 << 10, n_burn=(1 << 10) - 1,
                                want=("mom",))
    assert _raw(lib, x, flux, noise, n_chains=0) == -1 and b"n_chains must be at least 1" in lib.vamp_hmc_last_error()
    assert _raw(lib, x, flux, noise, start_flag=2) == -1 and b"start_is_device" in lib.vamp_hmc_last_error()
    assert _raw(lib, x, flux, noise, out_flag=2) == -1 and b"out_is_device" in lib.vamp_hmc_last_error()
    assert _raw(lib, x, flux, noise, groups=0) == -1 and b"n_groups" in lib.vamp_hmc_last_error()
    assert lib.vamp_hmc_chains(0, None, 1, *([None] * 11), None, 0, None, None, None, 4, 8, 0, 1, 0, 1, None, None, None, 0, *([None] * 12)) == -1
    assert b"NULL argument" in lib.vamp_hmc_last_error()
    # what Python refuses itself
    s, v = np.tile([1.0, 5.0, 1.5], (2, 1)), 0.1 * np.eye(3)
    with pytest.raises(ValueError, match="do not hold"):
        hmc.hmc_points(x, flux, noise, np.ones((2, 4)), v, 1, 0, 0.5)
    with pytest.raises(ValueError, match="does not belong"):
        hmc.hmc_points(x, flux, noise, s, np.eye(4), 1, 0, 0.5)
    with pytest.raises(ValueError, match="mode 2"):
        hmc.hmc_points(x, flux, noise, s, v, 1, 2, 0.5)
    with pytest.raises(ValueError, match="n_comp"):
        hmc.hmc_points(x, flux, noise, np.ones((2, 51)), np.eye(51), 17, 0, 0.5)
    with pytest.raises(ValueError, match="one abscissa"):
        hmc.hmc_points([x], [flux], [noise, noise], [s], [v], 1, 0, 0.5)
    with pytest.raises(ValueError, match="n_leap"):
        hmc.hmc_points(x, flux, noise, s, v, 1, 0, 0.5, n_leap=65)
    with pytest.raises(ValueError, match="n_burn"):
        hmc.hmc_points(x, flux, noise, s, v, 1, 0, 0.5, n_steps=4, n_burn=4)
    with pytest.raises(ValueError, match="unknown traces"):
        hmc.hmc_points(x, flux, noise, s, v, 1, 0, 0.5, want=("momentum",))
    with pytest.raises(ValueError, match="bounds must be"):
        hmc.hmc_points([x], [flux], [noise], [s], [v], 1, 0, 0.5, bounds=[(0.0, 1.0)])
    assert hmc.hmc_points([], [], [], [], [], 1, 0, 0.5) == [] and hmc.fits_hmc([]) == []


def _raw(lib, x, flux, noise, groups=1, n_chains=2, start_flag=0, out_flag=0):
    vp = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    i32 = lambda v: np.array([v], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    f64 = lambda v: np.array([v], dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    s, ch = np.tile([1.0, 5.0, 1.5], (2, 1)), 0.1 * np.eye(3)
    return lib.vamp_hmc_chains(0, None, groups, vp(x), vp(flux), vp(noise), i32(12), i32(1), i32(0), i32(0), None, i32(0), i32(n_chains), i32(0),
                               vp(s), start_flag, vp(ch), f64(0.5), f64(0.0), 4, 8, 0, 1, 0, 1, None, None, None, out_flag, *([None] * 12))


# ---- the Python wiring, the library call replaced by a fake ----------------------------------------------------------------
def test_python_helpers():
    from vamp_amd import hmc
    x = np.arange(24.0)
    lo, hi, wmax = hmc.derived_bounds(x, 0)
    assert (lo, hi, wmax) == (0.0, 23.0, 11.5) and hmc.derived_bounds(x[::-1], 1)[2] == pytest.approx(11.5 * 2 * math.sqrt(2 * math.log(2)))
    th = np.array([[1.0, 5.0, 1.5, 0.1], [0.0, 5.0, 1.5, 0.1], [1.0, 24.0, 1.5, 0.1], [1.0, 5.0, 0.0, 0.1], [1.0, 5.0, 1.5, 0.0], [1.0, 5.0, 1.5, 1.1],
                   [np.nan, 5.0, 1.5, 0.1]])
    assert list(hmc.inside_prior(th, 1, 0, True, lo, hi, wmax)) == [True, False, False, False, False, False, False]
    v = np.array([[1.0, 5.0, 0.0, 2.0], [1.0, 5.0, -0.1, 2.0], [1.0, 5.0, 1.0, 0.0]])
    assert list(hmc.inside_prior(v, 1, 1, False, lo, hi, 27.0)) == [True, False, False]
    # the library's own rule agrees
    R = evidence_ref.make_region(x, np.ones(24), None, 1, 0, True)
    assert [bool(evidence_ref.lnlike_lnprior(R, t)[1] > -np.inf and np.isfinite(evidence_ref.lnlike_lnprior(R, t)[0])) for t in th] == \
        list(hmc.inside_prior(th, 1, 0, True, lo, hi, wmax))
    rng = np.random.default_rng(0)
    inside = lambda t: hmc.inside_prior(t, 1, 0, True, lo, hi, wmax)
    s = hmc.draw_starts(np.array([0.05, 5.0, 1.5, 0.1]), np.diag([0.1, 0.1, 0.1, 0.01]), 64, rng, inside)
    assert s.shape == (64, 4) and inside(s).all() and len(np.unique(s[:, 0])) == 64
    assert np.allclose(hmc.tuned_eps([1.0, 1.0, 1.0], [0.9, 0.5, np.nan], 0.8), [1.5, 1 / 1.5, 1 / 1.5])
    rec = hmc.HmcRecord(chain=np.arange(24.0).reshape(2, 3, 4), last=np.ones((3, 4)), chain_status=np.array([0, 2, 0]), status=0, thin=1)
    assert rec.samples().shape == (4, 4) and rec.summary()[2].shape == (3, 4)
    moved = rec.to_units(np.full(4, 2.0), np.full(4, 1.0), names=list("abcd"))
    assert np.array_equal(moved.chain, rec.chain * 2 + 1) and moved.names == list("abcd") and np.array_equal(moved.last, np.full((3, 4), 3.0))
    with pytest.raises(ValueError, match="scales"):
        rec.to_units(np.ones(3))


class FakeHmc:
    """stands in for ``vamp_amd.hmc._call``: records the calls and answers with chains that sit on their starts"""

    def __init__(self, accept=0.9):
        self.seen, self.accept = [], accept

    def __call__(self, device, xs, fluxes, noises, n_comp, modes, sample_sd, bounds, region_ids, n_chains, chain_id0, starts, chols, eps, jitter,
                 n_leap, n_steps, n_burn=0, thin=1, step0=0, seed=0, want=(), **kw):
        from vamp_amd import hmc
        self.seen.append(dict(eps=np.array(eps, dtype=float), n_steps=n_steps, n_burn=n_burn, step0=step0, starts=[np.array(s) for s in starts],
                              chols=[np.array(c) for c in chols], seed=seed, region_ids=list(region_ids), want=tuple(want)))
        keep = hmc.n_keep_of(n_steps, n_burn, thin)
        bad = [not np.isfinite(np.tril(c)).all() for c in chols]
        tot = sum(n_chains)
        acc = self.accept(np.array(eps, dtype=float)) if callable(self.accept) else np.full(len(xs), self.accept)
        return {"chain": [np.tile(s, (keep, 1, 1)) * (np.nan if b else 1.0) for s, b in zip(starts, bad)],
                "last": [np.array(s) * (np.nan if b else 1.0) for s, b in zip(starts, bad)], "lnp": [np.zeros((keep, c)) for c in n_chains],
                "n_accept": np.concatenate([np.full(c, int(round(a * n_steps)), dtype=np.int32) for c, a in zip(n_chains, acc)]),
                "n_wall": np.zeros(tot, dtype=np.int32), "chain_status": np.concatenate([np.full(c, int(b), dtype=np.int32) for c, b in zip(n_chains, bad)]),
                "dH_mean": np.zeros(tot), "dH_max": np.zeros(tot), "status": np.array(bad, dtype=np.int32)}


def test_fits_hmc_tunes_then_runs_and_converts_units(monkeypatch):
    """six tuning calls and one kept call; eps moves towards the target acceptance by 1.5, 1.5, then 1.25; a fit whose Fisher
    status is not 0 gets status 1 and no chain; the record is in the caller's units"""
    import types
    from vamp_amd import fisher, hmc
    x = np.arange(24.0)
    fits = [types.SimpleNamespace(_x=x, _flux=np.ones(24), noise=np.full(24, 0.1), _sample_sd=False, _n=1, _mode=0, _scale=np.array([1.0, 2.0, 2.0]),
                                  _shift=np.array([0.0, 1000.0, 0.0]), _names=["A", "c", "s"], _theta_dev=np.array([1.0, 11.0, 2.0])) for _ in range(2)]
    cov = np.diag([0.01, 0.04, 0.04])
    recs = [types.SimpleNamespace(cov=cov * np.outer(f._scale, f._scale), status=s) for f, s in zip(fits, (0, 1))]
    monkeypatch.setattr(fisher, "fits_fisher", lambda fs, device=0: recs)
    fake = FakeHmc(accept=lambda eps: np.where(eps > 1.0, 0.5, 0.95))
    monkeypatch.setattr(hmc, "_call", fake)
    out = hmc.fits_hmc(fits, n_chains=8, n_steps=50, n_burn=10, seed=3)
    assert len(fake.seen) == 7 and [s["n_steps"] for s in fake.seen] == [40] * 6 + [50] and [s["step0"] for s in fake.seen] == list(range(0, 241, 40))
    e0 = 3 ** -0.25
    assert fake.seen[0]["eps"][0] == pytest.approx(e0) and fake.seen[1]["eps"][0] == pytest.approx(e0 * 1.5)
    assert fake.seen[2]["eps"][0] == pytest.approx(e0 * 1.5 / 1.5) and fake.seen[3]["eps"][0] == pytest.approx(e0 * 1.25)
    assert np.allclose(np.tril(fake.seen[0]["chols"][0]), np.diag([0.1, 0.2, 0.2])) and np.isnan(fake.seen[0]["chols"][1]).all()
    assert out[0].status == 0 and out[0].chain.shape == (40, 8, 3) and out[0].names == ["A", "c", "s"]
    assert abs(out[0].chain[:, :, 1].mean() - (11.0 * 2 + 1000.0)) < 1.0 and out[0].eps == pytest.approx(fake.seen[-1]["eps"][0])
    assert out[1].status == 1 and out[1].chain is None
    first = hmc.fits_hmc(fits[:1], n_chains=8, n_steps=50, n_burn=10, seed=3)[0]
    assert np.array_equal(first.chain, out[0].chain)                        # seeded starts
