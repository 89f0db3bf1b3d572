"""CPU tests of the relabelling that undoes label switching: the numpy restatement (tests/relabel_ref.py) -- its two
solvers against each other, a planted permutation, the planted error (a row-greedy assignment) against the optimality
bar of the GPU comparison, the near-tie cap on the very inputs the GPU test uses, the rounds checker on the restatement, the
conditions on its case table and five planted errors of the host loop that must each fail it --, the libvamp_relabel.so boundary
(build, exports, ctypes table, DESIGN's definitions, argument checks before any device call, the host header through a
stand-alone program) and the Python wiring (mcmc.relabel, stats / trace / diagnostics with relabel=True, fits_relabel,
Evidence.relabel, VPspectrum.relabel, do_vamp --relabel) with the library call replaced by the restatement."""
import ctypes as C
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

import relabel_ref as ref
from conftest import ROOT


# ---- the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6])
def test_brute_force_and_scipy_agree(K):
    rng = np.random.default_rng(100 + K)
    v = ref.lines(ref.prior_wide(rng, 300, K, 4), K, 4)
    C_ = ref.cost_matrices(v, ref.lines(ref.prior_wide(rng, 1, K, 4), K, 4)[0], np.array([1.0, 30.0, 15.0, 15.0]))
    pb, tb, gap = ref.assign_brute(C_)
    ps, ts = ref.assign_scipy(C_)
    B = ref.bar(C_)
    assert np.all(np.abs(tb - ts) <= B)
    clear = gap > 2 * B
    assert clear.mean() >= 0.99 and np.array_equal(pb[clear], ps[clear])
    for p in (pb, ps):
        assert np.array_equal(np.sort(p, axis=1), np.tile(np.arange(K), (300, 1)))
    ints = rng.integers(0, 5, (200, K, K)).astype(float)               # exact arithmetic, ties abound
    assert np.array_equal(ref.assign_brute(ints)[1], ref.assign_scipy(ints)[1])


@pytest.mark.parametrize("K", range(1, 33))
def test_planted_permutation_is_recovered(K):
    q = 3 + K % 2
    rng = np.random.default_rng(200 + K)
    th, r, perm = ref.planted(rng, 40, K, q, sd=1)
    got = ref.relabel(th, K, q - 3, 1, r, np.ones(q), 1)
    assert np.array_equal(got["perm"], perm)
    moved = ref.lines(got["chain"], K, q)
    assert np.all(np.abs(moved - r[None]) < 6.0)                       # every line back at its label: jitter 1, separation 10
    assert np.array_equal(got["chain"][:, -1], th[:, -1])
    assert got["n_switched"] == int((perm != np.arange(K)).any(axis=1).sum()) == got["n_changed"] and got["n_iter"] == 1


def test_rounds_converge_on_the_two_line_chain_and_restore_its_moments():
    rng = np.random.default_rng(300)
    chain, mixed, swapped = ref.two_line_chain(rng)
    N, W, _ = chain.shape
    start = chain[0, 1, :6].reshape(2, 3)                              # an unswapped walker's first sample
    got = ref.relabel(mixed, 2, 0, 1, start, None, 10)
    clean = ref.relabel(chain, 2, 0, 1, start, None, 10)
    assert 2 <= got["n_iter"] <= 3 and got["n_changed"] == 0
    np.testing.assert_allclose(got["label_sd"], clean["label_sd"], rtol=0, atol=1e-12 * 2.0)
    np.testing.assert_allclose(got["label_mean"], clean["label_mean"], rtol=0, atol=1e-12 * 2.0)
    np.testing.assert_array_equal(got["scale"], clean["scale"])        # pooled over the lines: a swap does not move it
    raw = mixed.reshape(-1, 7)[:, 1].std(ddof=1)
    assert raw > 1.8 * got["label_sd"][0, 1]                           # slot 0's centre without relabelling: both lines
    assert got["n_switched"] >= int(swapped.sum()) * N * 0.9
    one = ref.relabel(mixed, 2, 0, 1, start, None, 1)
    assert one["n_iter"] == 1 and one["n_changed"] == one["n_switched"] > 0


def test_bad_samples_and_counts():
    rng = np.random.default_rng(301)
    th = ref.prior_wide(rng, 30, 3, 3, sd=1)
    th[4, 5] = np.nan                  # a line parameter: bad
    th[9, -1] = np.nan                 # the sd only: not bad
    th[11, 0] = np.inf
    r = ref.lines(th, 3, 3)[0]
    got = ref.relabel(th, 3, 0, 1, r, None, 5)
    assert (got["n_used"], got["n_bad"]) == (28, 2)
    assert np.isnan(got["cost"][[4, 11]]).all() and np.isfinite(np.delete(got["cost"], [4, 11])).all()
    assert np.array_equal(got["perm"][[4, 11]], np.tile(np.arange(3), (2, 1)))
    np.testing.assert_array_equal(got["chain"][[4, 11]], th[[4, 11]])
    assert np.isnan(got["chain"][9, -1]) and np.isfinite(got["label_mean"]).all()
    none = ref.relabel(np.full((3, 7), np.nan), 2, 0, 1, np.zeros((2, 3)), None, 3)
    assert none["n_used"] == 0 and np.isnan(none["label_mean"]).all() and np.isnan(none["label_sd"]).all() and np.all(none["scale"] == 1.0)
    one = ref.relabel(th[:1], 3, 0, 1, r, None, 3)
    assert np.isfinite(one["label_mean"]).all() and np.isnan(one["label_sd"]).all()


# ---- the planted error the GPU comparison must see ----------------------------------------------------------------
def test_row_greedy_assignment_misses_the_bar_by_orders_of_magnitude():
    C3 = np.array([[[1.0, 2.0, 9.0], [1.0, 9.0, 9.0], [9.0, 9.0, 1.0]]])
    pg, tg = ref.assign_greedy_rows(C3)
    pb, tb, _ = ref.assign_brute(C3)
    assert (tg[0], tb[0]) == (11.0, 4.0) and list(pb[0]) == [1, 0, 2]
    assert (tg - tb)[0] / ref.bar(C3)[0] > 1e12
    rng = np.random.default_rng(302)
    _, mixed, _ = ref.crossing_chain(rng)
    start = mixed[0, 1, :6].reshape(2, 3)
    want = ref.relabel(mixed, 2, 0, 1, start, None, 1)
    bad = ref.relabel(mixed, 2, 0, 1, start, None, 1, solver=ref.assign_greedy_rows)
    C_ = want["costs"]
    excess = (ref.perm_cost(C_, bad["perm"]) - ref.perm_cost(C_, want["perm"])) / ref.bar(C_)
    print("row-greedy on the crossing chain: %d of %d samples differ, worst excess %.3g bars" % ((excess > 1).sum(), len(excess), excess.max()))
    assert (excess > 1e3).sum() >= 5 and excess.max() > 1e9 and bad["n_switched"] != want["n_switched"]


@pytest.mark.parametrize("K,q", ref.EXACT_CASES)
def test_near_ties_are_rare_on_the_inputs_of_the_exact_comparison(K, q):
    """the GPU test compares permutations exactly wherever second best - best > 2 B_s and may leave out 1 % of a case"""
    th, r = ref.exact_case(K, q)
    C_ = ref.cost_matrices(ref.lines(th, K, q), r, np.ones(q))
    _, _, gap = ref.assign_brute(C_)
    near = gap <= 2 * ref.bar(C_)
    print("K %d q %d: %d near ties of %d, smallest gap %.3g bars" % (K, q, near.sum(), len(gap), (gap / ref.bar(C_)).min()))
    assert near.mean() <= 0.01


# ---- every round of the iteration: the rounds checker on the restatement, and on planted errors --------------------------
_ROUNDS = {}


def _restated_rounds(case, given):
    """the rounds checker's result on the restatement, once per (case, scale)"""
    if (case, given) not in _ROUNDS:
        _ROUNDS[case, given] = ref.check_rounds(ref.restated_call(), ref.rounds_case(case, given), ref.rounds_label(case, given), ref.R_MAX)
    return _ROUNDS[case, given]


def test_crowded_chain_has_two_bad_samples_and_a_nan_in_an_sd_alone():
    th, start = ref.crowded_chain(np.random.default_rng(303), 130, 9, 4, 2.5, sd=1)
    assert th.shape == (130, 37) and start.shape == (9, 4) and np.array_equal(start, ref.lines(th, 9, 4)[0])
    assert list(np.flatnonzero(ref.bad_samples(th, 9, 4))) == [43, 86] and np.isnan(th[43, 35]) and np.isinf(th[86, 1])
    assert np.isnan(th[65, -1]) and np.isfinite(th[65, :-1]).all()
    centres = np.sort(ref.lines(np.delete(th, [43, 86], axis=0), 9, 4)[:, :, 1], axis=1).mean(axis=0)
    assert np.all(np.abs(np.diff(centres) - 2.5) < 0.5)                 # 2.5 jitters apart, shuffled in every sample
    assert (ref.relabel(th, 9, 1, 1, start, None, 1)["n_switched"]) > 100


@pytest.mark.parametrize("given", [True, False], ids=["given", "pooled"])
@pytest.mark.parametrize("case", ref.ROUNDS_CASES, ids=lambda c: "K%d-q%d-sd%d-sep%g" % c[:4])
def test_rounds_checker_passes_on_the_restatement(case, given):
    """chained one-round calls against one R-round call for every R <= R_MAX, every round to the solver's bar, the
    descent of J and the fixed point (relabel_ref.check_rounds), with the restatement in the library's place"""
    res = _restated_rounds(case, given)
    print("%s: stop %s, J %.6g -> %.6g in %d rounds, smallest gap %.3g bars" % (
        ref.rounds_label(case, given), res["stop"], res["J"][0], res["J"][-1], len(res["J"]), res["gap"]))
    assert res["stop"] is None or 2 <= res["stop"] <= ref.R_MAX
    assert all(b <= a for a, b in zip(res["J"], res["J"][1:]))          # the restatement's J falls without any margin here


def test_rounds_table_meets_the_conditions_the_gpu_comparison_relies_on():
    """the table covers K = 3 (q = 3 and 4), 6, 9, 17, 32, sd 0 and 1, S = 192 (K <= 6) | 130 and W > 1 with padded rows
    for every lane width; every lane width has a case that stops in 3 .. R_MAX rounds; a case does not stop within R_MAX;
    no best / second-best gap of any round is below 1e3 bars where brute force applies (every cost matrix finite:
    check_rounds asserts it)"""
    from vamp_amd import relabel
    assert ref.R_MAX <= 12 and relabel.DEFAULT_MAX_ITER <= ref.R_MAX
    cases = ref.ROUNDS_CASES
    assert {(c[0], c[1]) for c in cases} >= {(3, 3), (3, 4)} and {c[0] for c in cases} == {3, 6, 9, 17, 32} and {c[2] for c in cases} == {0, 1}
    assert all(c[5] == (192 if c[0] <= 6 else 130) and c[5] % c[6] == 0 for c in cases)
    width = lambda c: 8 if c[0] <= 8 else 16 if c[0] <= 16 else 32
    assert {width(c) for c in cases if c[6] > 1 and c[7] > 0} == {8, 16, 32}
    stops = {(c, gv): _restated_rounds(c, gv)["stop"] for c in cases for gv in (True, False)}
    assert {width(c) for (c, gv), st in stops.items() if st is not None and 3 <= st <= ref.R_MAX} == {8, 16, 32}
    assert any(st is None for (c, gv), st in stops.items() if c[0] in (17, 32))
    assert len({st for st in stops.values()}) >= 4                     # and they do not all stop in the same round
    for c in cases:
        for gv in (True, False):
            assert c[0] > ref.BRUTE_MAX_K or _restated_rounds(c, gv)["gap"] >= 1e3, c


# the assertion of relabel_ref.check_rounds (or of check_round inside it) that each planted error of relabel_ref.relabel breaks
_BREAKS = {
    "means through the inverse permutation": r"round 1', 'label_mean'",        # check_round: the moments under its own permutations
    "bad samples in the means' n": r"round 1', 'label_mean'",                  # the same assertion
    "reference not moved": r"closure: perm of 2 rounds in one call is not that of chained round 2",
    "prev never updated": r"closure: n_changed = \d+ after 2 rounds",
    "n_iter is the round limit": r"closure: n_iter = 5 after 5 rounds in one call, chained stop 4",
}


@pytest.mark.parametrize("plant", ref.PLANTS)
def test_rounds_checker_fails_on_a_planted_error(plant):
    case = ref.ROUNDS_CASES[1]                                         # K = 3, q = 4, W = 6 with padded rows: stops in round 4
    assert set(_BREAKS) == set(ref.PLANTS) and _restated_rounds(case, True)["stop"] == 4
    with pytest.raises(AssertionError, match=_BREAKS[plant]):
        ref.check_rounds(ref.restated_call(plant), ref.rounds_case(case, True), "planted", ref.R_MAX)


# ---- the library boundary ----------------------------------------------------------------------------------------
def _header_src(name="vamp_relabel.h"):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_functions(stem="relabel"):
    return sorted(set(re.findall(r"\b(vamp_%s[a-z0-9_]+)\s*\(" % ("" if stem == "hip" else stem + "_"), _header_src("vamp_%s.h" % stem))))


@pytest.fixture(scope="module")
def relabel_lib():
    import vamp_amd.build as vb
    return vb.build_relabel(verbose=False)


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted(set(re.findall(r"\bT (vamp_[a-z0-9_]+)\b", out)))


def test_library_builds_and_exports_the_header(relabel_lib):
    assert os.path.exists(relabel_lib)
    names = _header_functions()
    assert names == ["vamp_relabel_assign", "vamp_relabel_chains", "vamp_relabel_last_error", "vamp_relabel_version"]
    assert _exports(relabel_lib) == names


def test_build_makes_seven_libraries_and_leaves_the_other_six_alone():
    import vamp_amd.build as vb
    assert vb.build(verbose=False).endswith("libvamp_hip.so")
    for stem in ("hip", "diag", "post", "evid", "pred", "loo", "relabel"):
        path = os.path.join(ROOT, "vamp_amd", "libvamp_%s.so" % stem)
        assert os.path.exists(path), stem
        assert _exports(path) == _header_functions(stem), stem           # nm -D: what each header declares, nothing of another
    csrc = lambda f: os.path.join(vb.HERE, "csrc", f)
    inc = lambda f: os.path.join(vb.HERE, "..", "include", f)
    assert set(vb.RELABEL_DEPS) == {vb.RELABEL_SRC, csrc("side_call.hpp"), csrc("relabel_host.hpp"), inc("vamp_relabel.h")}
    assert vb.RELABEL_SRC == csrc("relabel.hip") and vb.RELABEL_OUT.endswith("libvamp_relabel.so")
    assert vb.RELABEL_FLAGS == vb.SIDE_FLAGS == ["--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-fvisibility=hidden"]
    assert vb.POST_FLAGS == vb.EVID_FLAGS == vb.PRED_FLAGS == vb.LOO_FLAGS == vb.SIDE_FLAGS
    includes = set(re.findall(r'#include "([^"]+)"', open(vb.RELABEL_SRC).read()))
    assert includes == {"../../include/vamp_relabel.h", "relabel_host.hpp", "side_call.hpp"}      # no evaluator
    assert "hip" not in re.sub(r"//.*", "", open(csrc("relabel_host.hpp")).read()).lower()          # plain C++
    voigt, lane, groups = csrc("voigt_math.hpp"), csrc("lane_group.hpp"), csrc("chain_groups.hpp")
    assert set(vb.DIAG_DEPS) == {vb.DIAG_SRC, csrc("side_call.hpp"), inc("vamp_diag.h")}
    assert set(vb.POST_DEPS) == {vb.POST_SRC, csrc("side_call.hpp"), lane, groups, voigt, inc("vamp_post.h")}
    assert set(vb.EVID_DEPS) == {vb.EVID_SRC, csrc("side_call.hpp"), lane, voigt, csrc("draws.hpp"), inc("vamp_evid.h")}
    assert set(vb.PRED_DEPS) == {vb.PRED_SRC, csrc("side_call.hpp"), lane, groups, csrc("pointwise_ll.hpp"), voigt, inc("vamp_pred.h")}
    assert set(vb.LOO_DEPS) == {vb.LOO_SRC, csrc("side_call.hpp"), lane, groups, csrc("pointwise_ll.hpp"), voigt, inc("vamp_loo.h")}
    assert inc("vamp_hip.h") in vb.DEPS and not any("relabel" in d for d in vb.DEPS)
    for name in ("vamp_hip.h", "vamp_diag.h", "vamp_post.h", "vamp_evid.h", "vamp_pred.h", "vamp_loo.h"):
        assert "vamp_relabel" not in open(inc(name)).read()
    src = open(inc("vamp_relabel.h")).read()
    assert re.search(r"#define VAMP_RELABEL_ABI_VERSION 1\b", src) and re.search(r"#define VAMP_RELABEL_MAX_COMPONENTS 32\b", src)


def test_design_carries_the_header_s_definitions_word_for_word():
    """the block from "Definitions." to "Everything is fp64." of the header, without the comment's " * ", is in DESIGN.md"""
    src = open(os.path.join(ROOT, "include", "vamp_relabel.h")).read()
    block = src[src.index(" * Definitions.\n"):src.index(" * - Everything is fp64.")]
    text = "".join(line[3:] if line.startswith(" * ") else line[2:] if line.startswith(" *") else line for line in block.splitlines(keepends=True))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert len(text.splitlines()) == 30 and text in design
    assert "## 14." in design and "- Everything is fp64." in design[design.index(text):]


_CTYPES = {"int": C.c_int, "void*": C.c_void_p, "const char*": C.c_char_p, "const double* const*": C.POINTER(C.c_void_p),
           "double* const*": C.POINTER(C.c_void_p), "uint8_t* const*": C.POINTER(C.c_void_p), "double*": C.POINTER(C.c_double),
           "const double*": C.POINTER(C.c_double), "uint8_t*": C.POINTER(C.c_uint8), "const int64_t*": C.POINTER(C.c_int64),
           "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32)}


def _header_prototypes():
    protos = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\**)\s*\b(vamp_relabel_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_src()):
        types_ = []
        for prm in params.split(","):
            prm = " ".join(prm.split())
            if prm in ("void", ""):
                continue
            types_.append(re.sub(r"\s*\*", "*", re.sub(r"\s*\b\w+$", "", prm)).replace("*const", "* const"))
        protos[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types_)
    return protos


def test_ctypes_table_mirrors_header():
    from vamp_amd import _relabel_lib
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() == sorted(_relabel_lib.SIGNATURES)
    ch = protos["vamp_relabel_chains"][1]
    assert len(ch) == 27 and ch[8] == "const int64_t*" and ch[11] == ch[12] == "const double* const*" and ch[14] == "double* const*"
    assert ch[17] == "uint8_t* const*" and ch[22:] == ["int32_t*"] * 5
    assert protos["vamp_relabel_assign"][1] == ["int", "int", "int", "const double*", "uint8_t*", "double*"]
    for name, (ret, params) in protos.items():
        res, args = _relabel_lib.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(args) == len(params), name
        for i, (ty, arg) in enumerate(zip(params, args)):
            assert arg is _CTYPES[ty] or arg == _CTYPES[ty], (name, i, ty, arg)


def test_arguments_are_checked_before_any_device_call(relabel_lib):
    """on a box without a GPU every call fails; these fail with the message of their check, not with "no HIP device" """
    from vamp_amd import _relabel_lib, relabel
    lib = _relabel_lib.load()
    assert lib.vamp_relabel_version() == 1
    chain = np.ones((10, 4, 7))
    out_far = np.ones((10, 4, 7))

    def call(n=10, W=4, K=2, mode=0, sd=1, ld=28, base=chain.ctypes.data, r=None, scale=None, max_iter=3, out=None, out_ld=28):
        r = np.ones((max(K, 0), 4 if mode == 1 else 3)) if r is None else r
        with pytest.raises(_relabel_lib.RelabelError) as e:
            relabel._call(0, [K], [mode], [sd], [base], False, [ld], [n], [W], [r], None if scale is None else [scale], max_iter,
                          None if out is None else [out], [out_ld], False)
        return str(e.value)

    assert "NULL base pointer" in call(base=None)
    assert "n_comp = 0 is outside 1 .. 32" in call(K=0)
    assert "n_comp = 33 is outside 1 .. 32" in call(K=33, ld=4 * 100)
    assert "mode 2 (NBZ3) is not supported" in call(mode=2)
    assert "mode must be" in call(mode=3)
    assert "ld < walkers * ndim" in call(ld=27)
    assert "ld < walkers * ndim" not in call(sd=0, ld=24, max_iter=0)
    for v in (np.nan, np.inf):
        r = np.ones((2, 3))
        r[1, 2] = v
        assert "ref is not finite at line 1, parameter 2" in call(r=r)
    for v in (0.0, -1.0, np.nan, np.inf):
        assert "scale is not finite and positive at parameter 1" in call(scale=np.array([1.0, v, 1.0]))
    assert "max_iter must be at least 1" in call(max_iter=0)
    assert "out overlaps base" in call(out=chain.ctypes.data + 8)
    assert "out overlaps base" in call(out=chain.ctypes.data, out_ld=29)          # the same start is not the same chain
    assert "out_ld < walkers * ndim" in call(out=out_far.ctypes.data, out_ld=27)
    assert "is not below 2^31" in call(n=1 << 16, W=1 << 15, ld=7 << 15)
    # what passes the checks reaches the device: in place, and out apart
    for kw in (dict(out=chain.ctypes.data), dict(out=out_far.ctypes.data), dict()):
        msg = call(**kw)
        assert "hipGetDeviceCount" in msg or "no HIP device" in msg, msg
    rest = [None] * 4 + [0] + [None] * 5 + [1, None, None, 0] + [None] * 10
    assert lib.vamp_relabel_chains(0, None, 0, *rest) == -1 and b"n_groups must be positive" in lib.vamp_relabel_last_error()
    assert lib.vamp_relabel_chains(0, None, 1, *rest) == -1 and b"NULL argument" in lib.vamp_relabel_last_error()
    with pytest.raises(ValueError):
        relabel.relabel_chains(np.zeros((4, 4)), 1, 0, 0, np.zeros((1, 3)))
    with pytest.raises(ValueError):
        relabel.relabel_chains(np.zeros((4, 4, 3)), 1, 0, 1, np.zeros((1, 3)))       # free sd: a Gaussian line has 4 parameters
    with pytest.raises(ValueError):
        relabel.relabel_chains(np.zeros((4, 4, 3)), 1, 0, 0, np.zeros((2, 3)))

    def solve(K, n, null=False):
        cost = np.ones(max(1, n * K * K))
        dp = C.POINTER(C.c_double)
        assert lib.vamp_relabel_assign(0, K, n, None if null else cost.ctypes.data_as(dp), None, None) == -1
        return lib.vamp_relabel_last_error().decode()

    assert "K = 0 is outside" in solve(0, 1) and "K = 33 is outside" in solve(33, 1) and "n must be positive" in solve(2, 0)
    assert "NULL cost" in solve(2, 3, null=True)
    assert "hipGetDeviceCount" in solve(2, 3) or "no HIP device" in solve(2, 3)
    with pytest.raises(ValueError):
        relabel.assign(np.zeros((3, 2, 3)))


# ---- the host header through a stand-alone program ------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rl") / "relabel_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "relabel_host.cpp")])

    def run(lines):
        res = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
        assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
        out = res.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


def test_host_header_lanes_tasks_and_layout(program):
    widths = program(["lanes %d" % K for K in range(1, 33)])
    assert widths == ["lanes %d" % (8 if K <= 8 else 16 if K <= 16 else 32) for K in range(1, 33)]
    assert program(["tasks 32 3 65 0 32", "tasks 8 1 9", "tasks 4 2 0 0"]) == \
        ["tasks 4 | 0 0 | 0 32 | 0 64 | 2 0", "tasks 2 | 0 0 | 0 8", "tasks 0"]
    # two groups: K 2 GAUSS3 sd 1 (D 7), 5 x 13 = 65 samples; K 9 VOIGT4 sd 0 (D 36), 129 x 1 samples
    got = program(["check 3 2  2 0 1 5 13 100 0 0 0  9 1 0 129 1 36 0 1 1"])[0]
    assert got == "ok 194 1291 120 42 7 | 65 7 3 8 0 0 0 0 0 | 129 36 4 16 65 130 12 6 3"      # 2 chunks x 6, 3 chunks x 36
    one = "2 0 1 5 13 91 %d %d %d"
    assert program(["check 3 1 " + one % (0, 0, k) for k in (1, 2)]) == ["ok 65 130 12 6 3 | 65 7 3 8 0 0 0 0 0"] * 2


def test_host_header_messages(program):
    one = "%d %d %d %d %d %d %d %d %d"
    cases = {
        "check 0 1 " + one % (2, 0, 1, 5, 13, 91, 0, 0, 0): "fn: max_iter must be at least 1",
        "check 1 1 " + one % (0, 0, 1, 5, 13, 91, 0, 0, 0): "fn: group 0: n_comp = 0 is outside 1 .. 32",
        "check 1 1 " + one % (33, 0, 1, 5, 13, 9100, 0, 0, 0): "fn: group 0: n_comp = 33 is outside 1 .. 32",
        "check 1 1 " + one % (2, 2, 1, 5, 13, 91, 0, 0, 0):
            "fn: group 0: mode 2 (NBZ3) is not supported: pass the chain in the GAUSS3 (0) or VOIGT4 (1) layout",
        "check 1 1 " + one % (2, 0, 2, 5, 13, 91, 0, 0, 0): "fn: group 0: sample_sd must be 0 or 1",
        "check 1 1 " + one % (2, 0, 1, 0, 13, 91, 0, 0, 0): "fn: group 0: n_keep and walkers must be positive",
        "check 1 1 " + one % (2, 0, 1, 65536, 32768, 7 * 32768, 0, 0, 0): "fn: group 0: n_keep * walkers = 2147483648 is not below 2^31",
        "check 1 1 " + one % (2, 0, 1, 5, 13, 90, 0, 0, 0): "fn: group 0: ld < walkers * ndim",
        "check 1 1 " + one % (2, 0, 1, 5, 13, 91, 1, 0, 0): "fn: group 0: NULL ref",
        "check 1 1 " + one % (2, 0, 1, 5, 13, 91, 2, 0, 0): "fn: group 0: ref is not finite at line 1, parameter 2",
        "check 1 1 " + one % (2, 0, 1, 5, 13, 91, 0, 2, 0): "fn: group 0: scale is not finite and positive at parameter 2",
        "check 1 1 " + one % (2, 0, 1, 5, 13, 91, 0, 0, 3):
            "fn: group 0: out overlaps base without being the same chain (in place: out = base and out_ld = ld)",
        "check 1 1 " + one % (2, 0, 1, 5, 13, 91, 0, 0, 4):
            "fn: group 0: out overlaps base without being the same chain (in place: out = base and out_ld = ld)",
        "check 1 2 " + one % (2, 0, 1, 5, 13, 91, 0, 0, 0) + " " + one % (2, 1, 1, 5, 13, 116, 0, 0, 0): "fn: group 1: ld < walkers * ndim",
        "assign 0 1 0": "fn: K = 0 is outside 1 .. 32",
        "assign 33 1 0": "fn: K = 33 is outside 1 .. 32",
        "assign 2 0 0": "fn: n must be positive",
        "assign 32 2097152 0": "fn: n K K is not below 2^31",
        "assign 2 3 1": "fn: NULL cost",
    }
    got = program(list(cases))
    assert got == ["error " + m for m in cases.values()]
    assert program(["assign 2 3 0", "assign 32 2097151 0", "check 1 1 " + one % (2, 0, 1, 32768, 65535, 7 * 65535, 0, 1, 2)])[:2] == ["ok", "ok"]


# ---- wiring, with the library call replaced by the restatement ----------------------------------------------------
@pytest.fixture
def fake_library(monkeypatch):
    from vamp_amd import relabel
    calls = []
    monkeypatch.setattr(relabel, "_relabel_host", ref.fake_relabel_host(calls))
    return calls


def _fake_diag_host(arrays, c, device):
    """a stand-in for the diagnostics call: a plain (unsplit) R-hat per parameter; the other outputs are constants"""
    r_hat = []
    for a in arrays:
        n = a.shape[0]
        with np.errstate(all="ignore"):
            w = a.var(axis=0, ddof=1).mean(axis=0)
            b = a.mean(axis=0).var(axis=0, ddof=1)
            r_hat.append(np.sqrt(((n - 1) / n * w + b) / w))
    r_hat = np.concatenate(r_hat)
    return np.ones_like(r_hat), np.full_like(r_hat, 100.0), r_hat, np.ones(r_hat.size, dtype=np.int32), np.ones(r_hat.size, dtype=bool)


def _fake_fit(chain, K, mode, sample_sd, start):
    """a stand-in for a sampled VPfit: device-unit chain, caller units = device units * scale + shift per parameter"""
    from vamp_amd.vpfits import _EnsembleMCMC
    q = 4 if mode else 3
    per_line = ([1.0, 2.0, 2.0, 2.0][:q], [0.0, 5.0, 0.0, 0.0][:q])
    scale = np.array(per_line[0] * K + [1.0] * int(sample_sd))
    shift = np.array(per_line[1] * K + [0.0] * int(sample_sd))
    names = [nm % k for k in range(K) for nm in (("xexp_%d", "est_centroid_%d", "est_L_%d", "est_G_%d") if mode else
                                                  ("xexp_%d", "est_centroid_%d", "est_sigma_%d"))] + ["sd"] * int(sample_sd)
    fit = types.SimpleNamespace(_chain_dev=chain, _n=K, _mode=mode, _sample_sd=bool(sample_sd), device=0, _scale=scale, _shift=shift,
                                _theta_dev=np.concatenate([np.ravel(start), [0.1] * int(sample_sd)]))
    fit._to_caller = lambda th: th * scale + shift
    mc = _EnsembleMCMC(fit)
    mc._flat, mc._names = fit._to_caller(chain.reshape(-1, chain.shape[2])), names
    if mode:
        for k in range(K):
            mc._derived["est_sigma_%d" % k] = ("est_G_%d" % k, lambda g: g / 2.3548)
    fit.mcmc = mc
    return fit


def _two_line_fit(seed=400):
    rng = np.random.default_rng(seed)
    chain, mixed, swapped = ref.two_line_chain(rng)
    return _fake_fit(mixed, 2, 0, 1, chain[0, 1, :6]), _fake_fit(chain, 2, 0, 1, chain[0, 1, :6]), swapped


def test_relabel_is_cached_and_off_by_default(fake_library, monkeypatch):
    from vamp_amd import diagnostics
    monkeypatch.setattr(diagnostics, "_diag_host", _fake_diag_host)
    fit, clean, swapped = _two_line_fit()
    before = {nm: dict(fit.mcmc.stats()[nm]) for nm in fit.mcmc.stats()}
    diag_before = fit.mcmc.diagnostics()
    trace_before = fit.mcmc.trace("est_centroid_0")[:]
    assert fake_library == []                                       # nothing so far has asked for a relabelling
    rec = fit.mcmc.relabel()
    assert fake_library == [(1, 10)] and fit.mcmc.relabel() is rec and fake_library == [(1, 10)]
    assert rec.converged and 2 <= rec.n_iter <= 3 and rec.n_changed == 0 and rec.perm.shape == (40, 16, 2) and rec.cost.shape == (40, 16)
    assert rec.perm.dtype == np.uint8 and rec.n_used == 640 and rec.n_bad == 0 and rec.chain is None
    assert fit.mcmc.relabel(max_iter=1) is not rec and fake_library == [(1, 10), (1, 1)]
    assert not fit.mcmc.relabel(max_iter=1).converged and fit.mcmc.relabel() is rec
    # without the keyword every result is what it was, to the byte
    after = {nm: dict(fit.mcmc.stats()[nm]) for nm in fit.mcmc.stats()}
    assert json.dumps(before, sort_keys=True, default=float) == json.dumps(after, sort_keys=True, default=float)
    assert fit.mcmc.diagnostics() == diag_before and np.array_equal(fit.mcmc.trace("est_centroid_0")[:], trace_before)
    # with it: the per-line numbers of the chain whose labels were never swapped
    want = clean.mcmc.stats()
    got = fit.mcmc.stats(relabel=True)
    for nm in got:
        assert got[nm]["standard deviation"] == pytest.approx(want[nm]["standard deviation"], rel=1e-12), nm
        assert got[nm]["mean"] == pytest.approx(want[nm]["mean"], rel=1e-12), nm
    assert before["est_centroid_0"]["standard deviation"] > 1.8 * got["est_centroid_0"]["standard deviation"]
    np.testing.assert_array_equal(fit.mcmc.trace("est_centroid_1", relabel=True)[:], clean.mcmc.trace("est_centroid_1")[:])
    np.testing.assert_array_equal(fit.mcmc.trace("sd", relabel=True)[:], fit.mcmc.trace("sd")[:])
    d = fit.mcmc.diagnostics(relabel=True)
    assert d["est_centroid_0"]["r_hat"] < 1.2 < diag_before["est_centroid_0"]["r_hat"]
    assert d == clean.mcmc.diagnostics() and fit.mcmc.diagnostics() == diag_before and fake_library == [(1, 10), (1, 1)]
    none = _fake_fit(fit._chain_dev, 2, 0, 1, np.zeros(6))
    none._chain_dev = None
    with pytest.raises(RuntimeError):
        none.mcmc.relabel()


def test_caller_units_are_mapped_after_gathering_when_the_lines_map_differently(fake_library):
    fit, clean, _ = _two_line_fit(401)
    for f in (fit, clean):
        f._scale[4] = 3.0                                           # line 1's centre in another unit than line 0's
        f.mcmc._flat = f._to_caller(f._chain_dev.reshape(-1, 7))
        f.mcmc._same_line_units = False
    got, want = fit.mcmc.stats(relabel=True), clean.mcmc.stats()
    for nm in ("est_centroid_0", "est_centroid_1", "est_sigma_1"):
        assert got[nm]["standard deviation"] == pytest.approx(want[nm]["standard deviation"], rel=1e-12)


def test_ingest_checks_that_every_line_maps_alike():
    """_ingest_chain's check, on a real VPfit's unit map (no device is touched: the DIC is skipped)"""
    from vamp_amd import vpfits
    fit = vpfits.VPfit.__new__(vpfits.VPfit)
    fit._n, fit._q, fit._ndim, fit._voigt = 2, 3, 7, False
    fit._names = ["xexp_0", "est_centroid_0", "est_sigma_0", "xexp_1", "est_centroid_1", "est_sigma_1", "sd"]
    fit._scale, fit._shift = np.array([1.0, 2.0, 2.0, 1.0, 2.0, 2.0, 1.0]), np.array([0.0, 5.0, 0.0, 0.0, 5.0, 0.0, 0.0])
    fit.mcmc = vpfits._EnsembleMCMC(fit)
    chain = np.random.default_rng(402).normal(size=(4, 8, 7))
    fit._ingest_chain(chain, np.zeros((4, 8)), np.zeros(8), 4, 4, 1.0, scored="skip", set_values=False)
    assert fit.mcmc._same_line_units is True and fit.mcmc._relabel == {}
    fit._shift[4] = 6.0
    fit._ingest_chain(chain, np.zeros((4, 8)), np.zeros(8), 4, 4, 1.0, scored="skip", set_values=False)
    assert fit.mcmc._same_line_units is False


def test_fits_relabel_is_one_call_and_fills_every_cache(fake_library):
    from vamp_amd import relabel
    rng = np.random.default_rng(403)
    a, _, _ = _two_line_fit(404)
    th, r, perm = ref.planted(rng, 24, 3, 4)
    b = _fake_fit(th.reshape(6, 4, 12), 3, 1, 0, r)
    none = types.SimpleNamespace(mcmc=None, _chain_dev=None)
    have, recs = relabel.fits_relabel([a, none, b])
    assert fake_library == [(2, 10)] and have == [a, b]
    assert a.mcmc.relabel() is recs[0] and b.mcmc.relabel() is recs[1] and fake_library == [(2, 10)]
    assert recs[1].perm.shape == (6, 4, 3) and recs[1].label_mean.shape == (3, 4) and recs[1].scale.shape == (4,)
    np.testing.assert_array_equal(recs[1].gather(b._chain_dev), ref.relabel(th, 3, 1, 0, r, None, 10)["chain"].reshape(6, 4, 12))
    sig = b.mcmc.stats(relabel=True)["est_sigma_2"]["mean"]                # a derived trace follows its source
    assert sig == pytest.approx(b.mcmc.stats(relabel=True)["est_G_2"]["mean"] / 2.3548)
    recs2 = relabel.relabel_chains([a._chain_dev], 2, 0, 1, [relabel.fit_reference(a)], return_chain=True, max_iter=4)
    assert fake_library[-1] == (1, 4) and recs2[0].chain.shape == a._chain_dev.shape
    np.testing.assert_array_equal(recs2[0].chain, recs[0].gather(a._chain_dev))
    assert relabel.fits_relabel([none]) == ([], []) and relabel.relabel_chains([], 1, 0, 0, []) == []


def test_evidence_relabel_takes_the_best_sample_as_reference(fake_library):
    from vamp_amd import evidence
    rng = np.random.default_rng(405)
    chain, mixed, swapped = ref.two_line_chain(rng, N=20, W=8)
    lnl = rng.normal(size=(20, 8))
    lnl[7, 3] = 50.0
    ev = evidence.Evidence(lnZ=0.0, betas=np.array([0.0, 1.0]), chain=mixed, chain_lnl=lnl)
    with pytest.raises(RuntimeError):
        ev.relabel()                                                # the layout of the chain is not known
    ev.n_comp, ev.mode, ev.sample_sd = 2, 0, True
    rec = ev.relabel()
    assert fake_library == [(1, 10)] and ev.relabel() is rec and rec.converged and rec.chain.shape == mixed.shape
    want = ref.relabel(mixed, 2, 0, 1, mixed[7, 3, :6].reshape(2, 3), None, 10)
    np.testing.assert_array_equal(rec.chain, want["chain"])
    assert rec.chain[:, :, 1].std() < 0.6 * mixed[:, :, 1].std()
    with pytest.raises(RuntimeError):
        evidence.Evidence(lnZ=0.0, betas=np.zeros(2)).relabel()


def _fake_spectrum(rng, tmp_path=None, VPspectrum=None):
    if VPspectrum is None:
        from vamp_amd.vpspectrum import VPspectrum
    spec = VPspectrum.__new__(VPspectrum)
    spec.wavelength_array, spec.flux_array, spec.region_pixels, spec.device = np.linspace(1210.0, 1220.0, 120), np.ones(120), [(10, 30), (50, 94)], 0
    chain, mixed, _ = ref.two_line_chain(rng)
    th, r, _ = ref.planted(rng, 24, 3, 3, sd=1)
    fits = [_fake_fit(mixed, 2, 0, 1, chain[0, 1, :6]), _fake_fit(th.reshape(6, 4, 10), 3, 0, 1, r)]
    spec.regions = [types.SimpleNamespace(fit=f, n=f._n, num_pixels=e - s, best_chi_squared=1.0) for f, (s, e) in zip(fits, spec.region_pixels)]
    if tmp_path is not None:
        spec.output_filename = str(tmp_path / "spectrum_9_gauss_")
    return spec


_SPECTRUM_KEYS = {"n_iter", "n_changed", "n_switched", "n_used", "n_bad", "converged", "n_comp", "max_r_hat_before", "max_r_hat_after",
                  "min_n_eff_before", "min_n_eff_after", "tau_reliable_before", "tau_reliable_after",
                  "label_mean", "label_sd", "line_region"}


def test_spectrum_relabel_layout(fake_library, monkeypatch):
    from vamp_amd import diagnostics
    monkeypatch.setattr(diagnostics, "_diag_host", _fake_diag_host)
    spec = _fake_spectrum(np.random.default_rng(406))
    out = spec.relabel()
    assert fake_library == [(2, 10)] and set(out) == _SPECTRUM_KEYS
    fits = [r.fit for r in spec.regions]
    assert list(out["n_comp"]) == [2, 3] and list(out["line_region"]) == [0, 0, 1, 1, 1] and out["label_mean"].shape == (5, 3)
    assert list(out["converged"]) == [1, 1] and out["converged"].dtype == np.int8 and out["n_switched"].dtype == np.int32
    assert list(out["n_used"]) == [640, 24] and list(out["n_bad"]) == [0, 0] and list(out["n_changed"]) == [0, 0]
    assert out["max_r_hat_after"][0] < 1.2 < out["max_r_hat_before"][0] and np.isfinite(out["max_r_hat_after"][1])
    for i, f in enumerate(fits):
        rec = f.mcmc.relabel()                                      # the one call filled each fit's cache
        rows = out["line_region"] == i
        np.testing.assert_array_equal(out["label_mean"][rows], rec.label_mean * f._scale[:3] + f._shift[:3])
        np.testing.assert_array_equal(out["label_sd"][rows], rec.label_sd * f._scale[:3])
        st = f.mcmc.stats(relabel=True)
        assert out["label_sd"][rows][0, 1] == pytest.approx(st["est_centroid_0"]["standard deviation"] * np.sqrt(rec.n_used / (rec.n_used - 1.0)), rel=1e-9)
    assert fake_library == [(2, 10)]
    assert list(out["min_n_eff_before"]) == list(out["min_n_eff_after"]) == [100.0, 100.0] and out["tau_reliable_after"].dtype == np.int8
    assert list(out["tau_reliable_before"]) == [1, 1]
    assert max(d["r_hat"] for d in fits[0].mcmc.diagnostics(relabel=True).values()) == out["max_r_hat_after"][0]      # the same record
    spec.relabel(max_iter=1)                                        # another number of rounds does not replace what relabel=True reads
    assert fake_library == [(2, 10), (2, 1)] and fits[0].mcmc.relabel().converged
    spec.regions[1].fit._chain_dev = None
    with pytest.raises(RuntimeError):
        spec.relabel()


def test_do_vamp_relabel_is_opt_in(fake_library, monkeypatch, tmp_path, capsys):
    """the file only with --relabel; the perf record has exactly the fields it had either way"""
    from vamp_amd import diagnostics, do_vamp, h5min, vpspectrum
    monkeypatch.setattr(diagnostics, "_diag_host", _fake_diag_host)
    made, real = [], vpspectrum.VPspectrum

    class Spec:
        def __new__(cls, *a, **kw):
            spec = _fake_spectrum(np.random.default_rng(407), tmp_path, real)
            spec.chi_limit, spec.flux_model, spec.voigt, spec.dtype = 1.5, {"difficult_fit": False}, False, 0
            spec.fit_spectrum = lambda batched=False: {}
            made.append(spec)
            return spec

    monkeypatch.setattr(vpspectrum, "VPspectrum", Spec)
    recs = []
    for flags in ([], ["--relabel"]):
        assert do_vamp.main([__file__, "1215.67", "--output_folder", str(tmp_path)] + flags) == 0
        printed = capsys.readouterr().out.splitlines()
        line = [ln for ln in printed if ln.startswith("vamp_perf ")]
        recs.append(json.loads(line[0][len("vamp_perf "):]))
        assert os.path.exists(tmp_path / "spectrum_9_gauss_relabel.h5") == bool(flags)
        extra = [json.loads(ln[len("vamp_relabel "):]) for ln in printed if ln.startswith("vamp_relabel ")]
        assert len(extra) == len(flags) and all(e["relabel_seconds"] >= 0 and e["regions_not_converged"] == 0 for e in extra)
        assert json.load(open(tmp_path / "spectrum_9_gauss_perf.json")) == recs[-1]
    assert set(recs[0]) == set(recs[1]) and fake_library == [(2, 10)]
    for k in set(recs[0]) - {"seconds", "diagnostics_seconds"}:
        assert recs[0][k] == recs[1][k], k
    back = h5min.read(str(tmp_path / "spectrum_9_gauss_relabel.h5"))
    want = made[1].relabel()
    assert set(back) == set(want) == _SPECTRUM_KEYS
    for k in want:
        np.testing.assert_array_equal(back[k], want[k])
        assert back[k].dtype == want[k].dtype, k


def test_do_vamp_relabel_keeps_the_perf_record_of_a_spectrum_with_a_region_without_a_chain(fake_library, monkeypatch, tmp_path, capsys):
    """--relabel cannot be done for a region that has no chain: the finished fit still gets its record and perf.json, the
    option says on stderr what it left out, and no relabel file is written"""
    from vamp_amd import diagnostics, do_vamp, vpspectrum
    monkeypatch.setattr(diagnostics, "_diag_host", _fake_diag_host)
    real = vpspectrum.VPspectrum

    class Spec:
        def __new__(cls, *a, **kw):
            spec = _fake_spectrum(np.random.default_rng(408), tmp_path, real)
            spec.chi_limit, spec.flux_model, spec.voigt, spec.dtype = 1.5, {"difficult_fit": False}, False, 0
            spec.fit_spectrum = lambda batched=False: {}
            spec.regions[1].fit._chain_dev = None
            return spec

    monkeypatch.setattr(vpspectrum, "VPspectrum", Spec)
    assert do_vamp.main([__file__, "1215.67", "--output_folder", str(tmp_path), "--relabel"]) == 0
    got = capsys.readouterr()
    assert len([ln for ln in got.out.splitlines() if ln.startswith("vamp_perf ")]) == 1 and "vamp_relabel " not in got.out
    assert "--relabel left out: relabel: 1 of 2 regions have no chain" in got.err
    assert os.path.exists(tmp_path / "spectrum_9_gauss_perf.json") and not os.path.exists(tmp_path / "spectrum_9_gauss_relabel.h5")
