"""CPU controls of tests/test_gpu_posterior_limits.py and tests/test_gpu_diag_limits.py: every case is what it claims
(LDS sizes, chunk sizes and counts, from the restated arithmetic of tests/side_limit_cases.py), the references alone meet
the bars the GPU comparisons use, and a planted error of the kind those comparisons exist for is seen by them."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.special import wofz

import chain_diag_ref as dref
import posterior_ref as pref
import side_limit_cases as sc
from conftest import ROOT
from oracle import vamp_oracle as vo


def test_post_eval_lds_sizes():
    assert sc.post_eval_lds_bytes(17, 300) == 64640 < sc.DEFAULT_LDS < sc.post_eval_lds_bytes(18, 300) == 68320
    assert sc.post_eval_lds_bytes(32, 129) == 119840 == sc.EVAL_MAX_LDS
    assert sc.post_eval_lds_bytes(4, 32) == 36480 and sc.group_lanes(4, 32) == 16
    for K in range(1, sc.POST_MAX_K + 1):
        for P in (1, 2, 31, 32, 33, 64, 65, 129, 300, 100000):
            lanes = sc.group_lanes(K, P)
            assert lanes == (16 if P <= 32 and K <= 4 else 64)
            assert sc.post_eval_lds_bytes(K, P) <= sc.EVAL_MAX_LDS, (K, P)
    # the wide form needs the raise exactly from K = 18 on
    assert [K for K in range(1, 33) if sc.post_eval_lds_bytes(K, 64) > sc.DEFAULT_LDS] == list(range(18, 33))


def test_posterior_cases_are_what_they_claim():
    big = sc.BIG_LDS
    assert max(sc.post_eval_lds_bytes(K, P) for _, K, P, *_ in big) == sc.EVAL_MAX_LDS
    assert sorted({P for m, K, P, *_ in big if K == 32}) == [2, 64, 65, 129] and all(m == 1 and sd == 1 for m, K, P, N, W, sd in big if K == 32)
    assert sorted({(m, N * W) for m, K, P, N, W, sd in big if K == 18}) == [(m, S) for m in (0, 1) for S in (64, 65, 129)]
    for i in sc.BIG_LDS_NARROW:                          # a 16-lane group between two K = 32 neighbours
        assert sc.group_lanes(big[i][1], big[i][2]) == 16 and big[i - 1][1] == 32 and big[i + 1][1] == 32
    assert {(big[i][1], big[i][2]) for i in sc.BIG_LDS_NARROW} == {(2, 20), (4, 32)}
    assert all(4 * K + sd == 129 for m, K, P, N, W, sd in big if K == 32)
    m, K, P, N, W, sd = sc.JUST_UNDER
    assert (K, P) == (17, 300) and sc.post_eval_lds_bytes(K, P) < sc.DEFAULT_LDS
    lanes = {(P, K): sc.group_lanes(K, P) for _, K, P, *_ in sc.NARROW_CORNER}
    assert lanes == {(32, 4): 16, (33, 4): 64, (32, 5): 64, (33, 5): 64} and len(sc.NARROW_CORNER) == 16
    assert {N * W for _, _, _, N, W, _ in sc.NARROW_CORNER} == {17, 20}
    assert len(sc.regime_lines()) == 64 and len(sc.regime_groups()) == 96
    x = sc.regime_x()
    assert x.size == 65 and np.all(np.diff(x) == 1.0)


def test_diag_chunks_are_what_the_cases_claim():
    assert [sc.diag_chunk(N) for N in (48, 49, 300, 1000, 1400, 2048, 2049, 4100, 8192)] == [64, 63, 12, 4, 2, 1, 3, 1, 1]
    assert 256 // 63 * 63 == 252                          # Wc = 63 does not divide the block: 252 of 256 threads active
    for name, (N, W, D, *_) in sc.MANY_CHUNKS.items():
        assert (sc.diag_chunk(N), sc.diag_nchunks(N, W)) == sc.MANY_CHUNKS_COUNTS[name]
        assert sc.diag_nchunks(N, W) > 64
    assert sc.MANY_CHUNKS["large-wc1-70"][0] > sc.DIAG_SMALL_N >= sc.MANY_CHUNKS["wc1-200"][0]
    N, W, D = sc.STUCK_SHAPE
    assert sc.diag_chunk(N) == 12 and sc.diag_nchunks(N, W) == 11 and W - 5 >= 10 * 12
    assert sc.diag_nchunks(1000, 5) == 2 and sc.diag_chunk(1000) + 1 == 5       # W = Wc + 1: a last chunk of one walker
    for (N, W, D), path in zip(sc.NONFINITE_SHAPES, (True, False)):
        assert (N <= sc.DIAG_SMALL_N) == path and sc.diag_nchunks(N, W) > 1
    shapes = sc.BOUNDARY_SHAPES
    i3 = [s[0] for s in shapes].index(3)                   # the group the host answers sits between device groups
    assert 0 < i3 < len(shapes) - 1 and min(s[0] for s in shapes if s[0] != 3) == 4
    assert {s[0] for s in shapes} >= {48, 49, 2048, 2049, 8192, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 200, 1000, 3}
    # every (N + 2 R) Wc tile fits the LDS the launch asks for
    for N in range(4, 8193):
        R, tile = (8, sc.DIAG_TILE_SMALL) if N <= sc.DIAG_SMALL_N else (16, sc.DIAG_TILE_LARGE)
        assert sc.diag_chunk(N) >= 1 and (N + 2 * R) * sc.diag_chunk(N) <= tile, N


def test_long_window_case_crosses_two_blocks_of_lags():
    N, W, D, rho, seed = sc.LONG_WINDOW
    win = dref.diagnostics(dref.ar1(np.random.default_rng(seed), N, W, D, rho))[3]
    assert np.all(win > 128), win


def test_stuck_case_reference():
    tau, n_eff, r_hat, window, reliable = dref.diagnostics(sc.stuck_chain())
    assert np.all(tau[:3] == np.inf) and np.all(n_eff[:3] == 0) and np.all(window[:3] == -1) and not reliable[:3].any()
    assert np.isfinite(r_hat[0]) and np.isfinite(r_hat[1]) and r_hat[2] == np.inf
    assert np.isfinite(tau[3]) and reliable[3]


@pytest.fixture(scope="module")
def H():
    so = os.path.join(ROOT, "tests", "host", "libvoigt_host.so")
    if not os.path.exists(so):
        import __graft_entry__ as ge
        ge.build()
    lib = C.CDLL(so)

    def f(x, y):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        out = np.empty_like(x)
        lib.voigt_H_host(C.c_int64(x.size), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out
    return f


def test_evaluator_meets_the_flux_bar_on_the_regime_sweep(H):
    """the host build of the evaluator against scipy's wofz at every (X, y) of the sweep: 1e-13 relative wherever
    w > 1e-300.  tau = A y sqrt(pi) w, so a flux moves by tau e^-tau 1e-13 <= 3.7e-14: the 1e-12 bar has a margin of 25"""
    X, y = sc.regime_points()
    assert X.size == 64 * 65 and y.min() == 0.0 and y.max() > 800 and X.max() > 5e4
    got = H(X, y)
    w = wofz(X + 1j * y).real
    keep = w > 1e-300
    assert keep.sum() > 0.6 * X.size
    err = np.abs(got[keep] - w[keep]) / w[keep]
    print("regime sweep: points", int(keep.sum()), "worst relative error of the evaluator", err.max())
    assert err.max() <= 1e-13
    assert np.all(got[~keep] <= 1e-300)
    # the oracle's optical depths at the sweep's amplitudes stay where tau e^-tau 1e-13 is the flux error: tau is finite
    for A, c, L, G in sc.regime_lines():
        tau = vo.voigt_function(sc.regime_x(), c, A, L, G)
        assert np.all(np.isfinite(tau)) and np.all(tau >= 0) and tau.max() <= A              # y sqrt(pi) w(iy) < 1


def test_nan_flux_case_gives_the_headers_answer_in_numpy():
    """one good sample with a NaN flux: numpy's answer is the header's (every statistic of a column that holds a NaN is NaN,
    n_bad = 0, n_used = 21).  Its second line's decrement sum is -inf (times the width): the mean is infinite, the sd NaN,
    and the quantile that lands on the infinite order statistic is NaN (inf - inf in numpy's interpolation) -- at p = 0
    for a positive width, at p = 1 for a negative one"""
    for width, edge in ((0.5, 0), (-0.5, -1)):
        x, chain, w = sc.nan_flux_group(width)
        assert not pref.bad_samples(chain.reshape(21, 8), 2, vo.MODE_VOIGT4).any()
        with np.errstate(all="ignore"):
            r = pref.summaries(x, chain, 2, vo.MODE_VOIGT4, probs=sc.PROBS, pixel_width=w)
        assert (r["n_used"], r["n_bad"]) == (21, 0)
        for name in ("flux_mean", "flux_sd", "flux_q", "ew_mean", "ew_sd", "ew_q"):
            assert np.all(np.isnan(r[name])), name
        assert np.all(np.isfinite(r["comp_ew_mean"][0])) and np.all(np.isfinite(r["comp_ew_q"][0])) and np.isfinite(r["comp_ew_sd"][0])
        assert r["comp_ew_mean"][1] == -np.sign(width) * np.inf and np.isnan(r["comp_ew_sd"][1])
        q = r["comp_ew_q"][1]
        assert np.isnan(q[edge]) and not np.isfinite(q[1 if edge == 0 else -2]) and np.all(np.isfinite(q[2:-2]))


def test_offset_cases_k_is_the_largest_the_restatement_carries():
    """the float64 restatement against direct sums in np.longdouble on the parameter that is moved by 10^k: within 1e-10 at
    the table's k, outside at k + 1.  So at k the restatement is a yardstick for the kernel's 1e-9, and a larger offset would
    test the restatement, not the kernel"""
    for name, (N, W, D, seed, d, k, at_k, above) in sc.MANY_CHUNKS.items():
        a, b = sc.offset_agreement(name, k), sc.offset_agreement(name, k + 1)
        print("offset case", name, "k", k, "agreement", a, "at k + 1", b, "(table:", at_k, above, ")")
        assert a <= sc.OFFSET_RTOL < b, (name, a, b)
        assert at_k <= sc.OFFSET_RTOL < above and 0.1 < a / at_k < 10 and 0.1 < b / above < 10      # the table's figures: same order


def test_a_wrong_count_in_the_merge_of_65_chunks_is_seen():
    """numpy copy of the two kernels' R-hat path on the 65-chunk case (Welford per chunk, per-lane merges, shuffle tree):
    it agrees with the restatement to the GPU test's 1e-9, and with lane 0's merge of chunks 0 and 64 leaving the wrong
    count behind (that of chunk 0 alone) it misses that bar by orders of magnitude"""
    name = "wc2-65"
    d = sc.MANY_CHUNKS[name][4]
    x = sc.many_chunks_chain(name)[:, :, d]
    want = sc.many_chunks_want(name)[2][d]
    good, planted = sc.finish_r_hat(x), sc.finish_r_hat(x, wrong_lane=0)
    print("r_hat", want, "copy", abs(good / want - 1), "planted", abs(planted / want - 1))
    assert abs(good / want - 1) <= 1e-9
    assert abs(planted / want - 1) >= 1e-9 * 1e2           # (measured: 3.1e-7, 310 bars, for one of 65 chunks miscounted)


def test_a_dropped_summing_lane_is_seen():
    """numpy copy of k_post_eval's decrement sums on a K = 32, P = 129 sample: K + 1 = 33 summing lanes give the
    restatement's equivalent widths within the bar 1e-12 P |width|; with the 33rd lane dropped the region's equivalent
    width misses it by orders of magnitude"""
    m, K, P, N, W, sd = sc.BIG_LDS[5]
    assert (K, P) == (32, 129)
    x, chain = sc.drawn_group(np.random.default_rng(5), P, K, m, 1, 1, sd)
    want = pref.summaries(x, chain, K, m, bool(sd), sc.PROBS, 1.0)
    tau = pref.sample_taus(x, chain.reshape(1, -1), K, m)[0]
    bar = 1e-12 * P
    good, planted = sc.decrement_sums(tau), sc.decrement_sums(tau, owners=K)
    assert np.max(np.abs(good[:K] - want["comp_ew_mean"])) <= bar and abs(good[K] - want["ew_mean"]) <= bar
    assert abs(planted[K] - want["ew_mean"]) >= 1e6 * bar
