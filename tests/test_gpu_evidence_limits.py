"""GPU tests (-m gpu) of libvamp_evid.so at its structural limits, beside tests/test_gpu_evidence.py: the branches of
evidence.hip that the small shapes there never reach.

  1  one-region trajectories against the numpy restatement (tests/evidence_ref.py) where the kernels change path: dynamic
     LDS above and just below 64 KiB, a 16-lane group that takes a second and third round of movers, the narrow shape at its
     corner, ladders of 33 and 64 rungs with a short last launch and a burn off the swap grid, walker ids above 2^32 in the
     draw keys, the caller's own ladder and stretch scale.  Bars: those of test_trajectory_matches_the_restatement.
  2  k_evid_reduce alone, on runs longer than the restatement can follow: the device's own ln L trace goes through
     ref.reduce.  The bar of the block standard error is derived in evidence_cases.se_bar; tests/test_evidence_limits.py
     shows on the CPU that it can fail.
  3  vamp_evid_lnlike at the narrow / wide border, over several workgroups with a ragged tail, over twelve decades of Voigt
     damping, and at the exact edges L = 0, G = 0, sigma = 0, sd = 0.
  4  the arguments nobody passed: a stream, device chains of several regions, the order of a batch.

The device is never compared with a value the device produced, except where a test says bit-identical."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
from scipy.special import wofz

import evidence_ref as ref
from evidence_cases import (DEFAULT_LDS, LIMIT_CASES, SEED, as_dict, check_lnlike, limit_case, limit_region, se_bar, steps_lds_bytes,
                            synthetic)
from oracle import vamp_oracle as vo

pytestmark = pytest.mark.gpu

FIELDS = ("chain", "chain_lnl", "lnl_trace", "swap_trace", "mean_lnL", "var_lnL", "move_accept", "swap_accept", "lnZ", "lnZ_se", "lnZ_ti")


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k)), equal_nan=True) for k in FIELDS)


# ---- 1. trajectories at the structural limits -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want(name):
    R, betas, W, steps, burn, swap_every, rid, a = limit_case(name)
    return ref.run([R], [rid], betas, W, steps, burn, swap_every, SEED, a=a)[0]


def _run_case(name):
    from vamp_amd import evidence
    R, betas, W, steps, burn, swap_every, rid, a = limit_case(name)
    own = not isinstance(LIMIT_CASES[name][4], int)
    return evidence.log_evidence(as_dict(R, rid, bounds=False), n_temps=betas.size, betas=betas if own else None, walkers=W, steps=steps,
                                 burn=burn, swap_every=swap_every, seed=SEED, a=a, return_chain=True, trace=True)


_got = functools.lru_cache(maxsize=None)(_run_case)


def test_the_lds_premise():
    """the two 256-walker cases sit on either side of what a launch gets by default"""
    big, under = (steps_lds_bytes(*LIMIT_CASES[k][:4], LIMIT_CASES[k][5]) for k in ("big-lds", "just-under"))
    assert big == 85808 and under == 55824 and under < DEFAULT_LDS < big
    assert steps_lds_bytes(24, 2, 0, False, 66) == 6800                  # 16-lane groups: sixteen slots of 20 doubles


@pytest.mark.parametrize("name", list(LIMIT_CASES))
def test_trajectory_at_a_limit(name):
    R, betas, W, steps, burn, swap_every, rid, a = limit_case(name)
    T, n_keep, n_swaps = betas.size, steps - burn, (steps - 1) // swap_every
    w, d = _want(name), _got(name)
    assert w["move_accept"].sum() > 0 and w["swap_trace"].sum() > 0      # the restatement accepted moves and swaps
    assert d.chain.shape == (n_keep, W, R.ndim) and d.lnl_trace.shape == (n_keep, T, W) and d.swap_trace.shape == (n_swaps, T - 1, W)
    print(name, "lnZ", d.lnZ, w["lnZ"], "se", d.lnZ_se, w["lnZ_se"], "ti", d.lnZ_ti, w["lnZ_ti"],
          "max |d trace|", np.abs(d.lnl_trace - w["lnl_trace"]).max())
    assert np.array_equal(d.swap_trace, w["swap_trace"])
    np.testing.assert_allclose(d.lnl_trace, w["lnl_trace"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(d.chain, w["chain"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(d.chain_lnl, w["chain_lnl"], rtol=1e-10, atol=1e-12)
    np.testing.assert_array_equal(d.chain_lnl, d.lnl_trace[:, -1])
    np.testing.assert_allclose(d.move_accept, w["move_accept"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(d.swap_accept, w["swap_accept"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(d.mean_lnL, w["mean_lnL"], rtol=1e-10)
    np.testing.assert_allclose(d.var_lnL, w["var_lnL"], rtol=1e-8, atol=1e-12)
    assert d.lnZ == pytest.approx(w["lnZ"], rel=1e-9, abs=1e-9) and d.lnZ_ti == pytest.approx(w["lnZ_ti"], rel=1e-9, abs=1e-9)
    np.testing.assert_array_equal(d.betas, betas)
    if n_keep >= ref.N_BLOCKS:
        assert math.isfinite(w["lnZ_se"]) and abs(d.lnZ_se - w["lnZ_se"]) <= se_bar(w["zb"])
    else:
        assert math.isnan(d.lnZ_se) and math.isnan(w["lnZ_se"])


def test_big_lds_again_after_a_small_ladder_is_bit_identical():
    """the LDS limit is raised once per process and device: a launch above 64 KiB gives the same bits the first time, and
    again after a launch that never needed the raise"""
    first = _got("big-lds")
    small = _run_case("high-id")
    again = _run_case("big-lds")
    assert _same_bits(first, again)
    assert _same_bits(small, _got("high-id"))


# ---- 2. the reductions, decoupled from the trajectory ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_regions():
    return limit_region(17, 1, 0, False), limit_region(24, 2, 1, True)         # D = 3 and D = 9


def _check_reductions(rec, betas, W, steps, burn, swap_every, tag):
    """the outputs of k_evid_reduce against ref.reduce of the trace the device returned.  lnZ_se: |se - se_ref| <=
    1e-9 max(1, max_b |zb_ref|).  Each block estimate is the functional ln Z is, so it agrees to the project's bar of ln Z,
    1e-9 max(1, |zb|); the sample standard deviation of 8 values over sqrt 8 moves by at most max |delta zb| / sqrt 7
    (evidence_cases.se_bar), which is below that."""
    n_keep, n_swaps, T = steps - burn, (steps - 1) // swap_every, betas.size
    assert rec.lnl_trace.shape == (n_keep, T, W) and rec.swap_trace.shape == (n_swaps, T - 1, W)
    want = ref.reduce(rec.lnl_trace, betas)
    print(tag, "lnZ", rec.lnZ, want["lnZ"], "se", rec.lnZ_se, want["lnZ_se"], "ti", rec.lnZ_ti, want["lnZ_ti"])
    assert rec.lnZ == pytest.approx(want["lnZ"], rel=1e-9, abs=1e-9), tag
    assert rec.lnZ_ti == pytest.approx(want["lnZ_ti"], rel=1e-9, abs=1e-9), tag
    np.testing.assert_allclose(rec.mean_lnL, want["mean_lnL"], rtol=1e-10, err_msg=str(tag))
    np.testing.assert_allclose(rec.var_lnL, want["var_lnL"], rtol=1e-8, err_msg=str(tag))
    offered = np.array([(n_swaps + 1) // 2 if j % 2 == 0 else n_swaps // 2 for j in range(T - 1)], dtype=np.float64)
    assert offered.min() > 0
    np.testing.assert_array_equal(rec.swap_accept, rec.swap_trace.sum(axis=(0, 2)) / (offered * W), err_msg=str(tag))
    assert rec.swap_trace.sum() > 0 and np.all((rec.move_accept > 0) & (rec.move_accept < 1)), tag
    if n_keep < ref.N_BLOCKS:
        assert math.isnan(rec.lnZ_se) and want["zb"] is None, tag
    else:
        assert math.isfinite(rec.lnZ_se) and abs(rec.lnZ_se - want["lnZ_se"]) <= se_bar(want["zb"]), (tag, rec.lnZ_se, want["lnZ_se"])


@pytest.mark.parametrize("steps,burn,W", [(27, 20, 32), (28, 20, 32), (35, 20, 32), (100, 20, 32), (103, 20, 32), (103, 20, 6)],
                         ids=["keep7", "keep8", "keep15", "keep80", "keep83", "keep83-w6"])
def test_reductions_of_the_devices_own_trace(steps, burn, W):
    """n_keep = 7: no standard error; 8 and 80: equal blocks; 15 and 83: unequal blocks; W = 6: n_keep W = 498 is no multiple
    of the workgroup"""
    from vamp_amd import evidence
    regions = _two_regions()
    betas = ref.default_betas(16)
    recs = evidence.log_evidence([as_dict(R, 20 + g, bounds=False) for g, R in enumerate(regions)], n_temps=16, walkers=W, steps=steps,
                                 burn=burn, swap_every=5, seed=SEED, trace=True)
    for g, rec in enumerate(recs):
        _check_reductions(rec, betas, W, steps, burn, 5, (steps, burn, W, g))


# ---- 3. vamp_evid_lnlike at its borders -------------------------------------------------------------------------
@pytest.mark.parametrize("P", [31, 32, 33])
def test_lnlike_on_both_sides_of_the_narrow_border(P):
    """16-lane groups serve P <= 32 with K <= 4, whole wavefronts the rest"""
    for K in (4, 5):
        for mode in (0, 1):
            for sd in (False, True):
                R, theta = synthetic(P, K, mode, sd)
                assert check_lnlike(R, theta, True, (P, K, mode, sd)) >= 25


@pytest.mark.parametrize("P,K,mode,sd", [(24, 2, 0, False), (65, 2, 1, True)], ids=["16-lanes", "64-lanes"])
def test_lnlike_row_counts(P, K, mode, sd):
    """1 .. 200 rows in one call: up to four workgroups of 64 rows, the last one ragged; and row i of the longest call has the
    bits of the same vector evaluated alone"""
    from vamp_amd import evidence
    R, theta40 = synthetic(P, K, mode, sd)
    theta = np.concatenate([theta40] + [ref.prior_draws(R, 50 + j, 40, SEED) for j in range(4)])
    assert theta.shape[0] == 200
    spec = as_dict(R)
    alone = np.array([[v[0] for v in evidence.lnlike(spec, theta[i])] for i in range(200)])          # [200, (ln L, ln pi)]
    for n in (1, 63, 64, 65, 200):
        assert check_lnlike(R, theta[:n], True, (P, K, mode, sd, n)) >= min(n, 1)
        ll, lp = evidence.lnlike(spec, theta[:n])
        assert np.array_equal(ll, alone[:n, 0], equal_nan=True) and np.array_equal(lp, alone[:n, 1]), n


def _damping_region(K):
    """65 pixels one apart, noise 0.05, explicit bounds whose fwhm_max admits L_fwhm = 6e4"""
    R, _ = synthetic(65, K, 1, False)
    return ref.make_region(R.x, R.flux, R.noise, K, 1, False, bounds=(R.c_lo, R.c_hi, R.sigma_max, 1.0e5))


def _damping_vectors(R):
    """L_fwhm / G_fwhm over twelve decades times G_fwhm from a twentieth of a pixel to the region's width, centres on a pixel
    and between two.  The amplitude brings the line's depth at its centre to 1 where the prior allows (A <= 500)."""
    ratios, widths = (1e-12, 1e-6, 1e-3, 0.1, 1.0, 10.0, 1e3), (0.05, 1.0, 10.0, 60.0)
    rows = []
    for r in ratios:
        for G in widths:
            for c in (R.x[30], R.x[30] + 0.5):
                peak = r * math.sqrt(math.pi) * vo.SQRT_LN2 * wofz(1j * r * vo.SQRT_LN2).real        # tau at the centre for A = 1
                rows.append((min(500.0, max(0.3, 1.0 / peak)), c, r * G, G))
    rows = np.array(rows)
    if R.n_comp == 1:
        return rows
    return np.concatenate([rows, rows[::-1] * np.array([0.5, 1.0, 1.0, 1.0]) + np.array([0.0, 7.25, 0.0, 0.0])], axis=1)


@pytest.mark.parametrize("K", [1, 2])
def test_lnlike_over_the_voigt_damping(K):
    """y = L sqrt(ln 2) / G runs from 8e-13 to 8e2 and x up to 2e3: inside the range where tests/test_voigt_properties.py
    holds the evaluator to 1e-13 of scipy, so the oracle alone carries the 1e-9 bar.  evidence.hip stages the line records and
    the near-axis tables itself"""
    R = _damping_region(K)
    theta = _damping_vectors(R)
    assert theta.shape == (56, 4 * K)
    assert check_lnlike(R, theta, True, ("damping", K)) == 56


def test_lnlike_at_the_gaussian_limit():
    """L_fwhm = 0: y = 0, the line has no depth in this parametrisation (amplitude of the Lorentzian), and ln L is finite"""
    for K in (1, 2):
        R = _damping_region(K)
        theta = _damping_vectors(R)[8:24].copy()
        theta[:, 2] = 0.0
        if K == 2:
            theta[::2, 6] = 0.0
        assert check_lnlike(R, theta, True, ("L = 0", K)) == 16


def test_degenerate_widths_are_rejected_by_both():
    """G_fwhm = 0, sigma = 0 and sd = 0 lie inside the prior's closed ranges and have no ln L.  Device and oracle both give the
    tempered target -inf, through different outputs: the device reports a zero width like a point outside the prior
    (ln pi = -inf, ln L NaN, not evaluated), the oracle keeps ln pi and has no finite ln L; sd = 0 is ln L = -inf on both.
    (sigma = 0 with the centre between two pixels is the one place where the oracle's arithmetic gives a number -- a line of
    no width that no pixel sees --; the device rejects every zero width, so the centre sits on a pixel here.)"""
    from vamp_amd import evidence
    Rv, Rg, Rs = _damping_region(1), synthetic(65, 1, 0, False)[0], synthetic(65, 1, 0, True)[0]
    on, off = Rv.x[30], Rv.x[30] + 0.5
    cases = [(Rv, [1.0, on, 1.0, 0.0]), (Rv, [1.0, off, 1.0, 0.0]), (Rv, [1.0, on, 0.0, 0.0]), (Rg, [1.0, on, 0.0])]
    for R, th in cases:
        th = np.array(th)
        (ll,), (lp,) = evidence.lnlike(as_dict(R), th)
        wll, wlp = ref.lnlike_lnprior(R, th)
        assert lp == -np.inf and math.isnan(ll), th                      # the device's pattern
        assert math.isfinite(wlp) and wll == -np.inf, th                 # the oracle's
        for beta in (0.0, 0.3, 1.0):
            assert ref.target(lp, ll, beta) == -np.inf and ref.target(wlp, wll, beta) == -np.inf
    th = np.array([1.0, on, 2.0, 0.0])
    (ll,), (lp,) = evidence.lnlike(as_dict(Rs), th)
    wll, wlp = ref.lnlike_lnprior(Rs, th)
    assert ll == -np.inf and wll == -np.inf and lp == pytest.approx(wlp, rel=1e-9) and math.isfinite(wlp)
    assert ref.target(lp, ll, 0.5) == -np.inf
    check_lnlike(Rs, th[None], True, "sd = 0")


# ---- 4. arguments nobody passes ---------------------------------------------------------------------------------
def _raw_run(regions, ids, T=3, W=6, steps=7, burn=2, swap_every=2, stream=None, device_chain=False, no_chain=()):
    """one vamp_evid_run through ctypes; per region a dict of every output.  ``no_chain``: regions with NULL chain entries"""
    import torch
    from vamp_amd import _evid_lib
    lib = _evid_lib.load()
    G, n_keep, n_swaps = len(regions), steps - burn, (steps - 1) // swap_every
    dp = C.POINTER(C.c_double)
    vp = lambda seq: (C.c_void_p * G)(*seq)
    i32 = lambda seq: np.ascontiguousarray(seq, dtype=np.int32)
    n_pix, n_comp, modes, sds, rid = (i32(v) for v in ([R.x.size for R in regions], [R.n_comp for R in regions], [R.mode for R in regions],
                                                       [int(R.sample_sd) for R in regions], ids))
    out = {k: np.full(n, np.nan) for k, n in (("lnZ", G), ("lnZ_se", G), ("lnZ_ti", G), ("mean_lnL", G * T), ("var_lnL", G * T),
                                              ("move_accept", G * T), ("swap_accept", G * (T - 1)))}
    trace = np.full((G, n_keep, T, W), np.nan)
    swaps = np.zeros((G, n_swaps, T - 1, W), dtype=np.uint8)
    if device_chain:
        chains = [None if g in no_chain else torch.zeros((n_keep, W, R.ndim), dtype=torch.float64, device="cuda") for g, R in enumerate(regions)]
        clls = [None if g in no_chain else torch.zeros((n_keep, W), dtype=torch.float64, device="cuda") for g in range(G)]
        torch.cuda.synchronize()
        addr = lambda t: None if t is None else t.data_ptr()
    else:
        chains = [None if g in no_chain else np.zeros((n_keep, W, R.ndim)) for g, R in enumerate(regions)]
        clls = [None if g in no_chain else np.zeros((n_keep, W)) for g in range(G)]
        addr = lambda a: None if a is None else a.ctypes.data
    noise = [None if R.sample_sd else R.noise for R in regions]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.vamp_evid_run(0, stream, G, vp([R.x.ctypes.data for R in regions]), vp([R.flux.ctypes.data for R in regions]),
                           vp([None if a is None else a.ctypes.data for a in noise]), ip(n_pix), ip(n_comp), ip(modes), ip(sds), None, ip(rid),
                           T, None, W, steps, burn, swap_every, SEED, 2.0, None, *[out[k].ctypes.data_as(dp) for k in
                                                                                   ("lnZ", "lnZ_se", "lnZ_ti", "mean_lnL", "var_lnL", "move_accept", "swap_accept")],
                           vp([addr(c) for c in chains]), vp([addr(c) for c in clls]), int(device_chain), trace.ctypes.data_as(dp),
                           swaps.ctypes.data_as(C.POINTER(C.c_uint8)))
    _evid_lib.check(rc, lib)
    if device_chain:
        torch.cuda.synchronize()
        chains, clls = ([None if t is None else t.cpu().numpy() for t in seq] for seq in (chains, clls))
    recs = []
    for g in range(G):
        rec = {k: out[k][g] for k in ("lnZ", "lnZ_se", "lnZ_ti")}
        rec.update({k: out[k][g * T:(g + 1) * T] for k in ("mean_lnL", "var_lnL", "move_accept")})
        rec.update(swap_accept=out["swap_accept"][g * (T - 1):(g + 1) * (T - 1)], chain=chains[g], chain_lnl=clls[g], lnl_trace=trace[g],
                   swap_trace=swaps[g])
        recs.append(rec)
    return recs


def _assert_same(a, b, tag, chain=True):
    for k in a:
        if k in ("chain", "chain_lnl") and (not chain or a[k] is None or b[k] is None):
            continue
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (tag, k)


@functools.lru_cache(maxsize=None)
def _three_regions():
    return limit_region(17, 1, 0, False), limit_region(24, 2, 1, True), limit_region(40, 3, 0, True)      # D = 3, 9, 10


THREE_IDS = (11, 3, 40)


@functools.lru_cache(maxsize=None)
def _three_host():
    return _raw_run(_three_regions(), THREE_IDS)


def test_the_host_batch_follows_the_restatement():
    """what the three tests below compare with bit for bit is itself the restatement's trajectory"""
    want = ref.run(_three_regions(), THREE_IDS, ref.default_betas(3), 6, 7, 2, 2, SEED)
    for g, (w, d) in enumerate(zip(want, _three_host())):
        assert w["move_accept"].sum() > 0
        assert np.array_equal(d["swap_trace"], w["swap_trace"]), g
        np.testing.assert_allclose(d["lnl_trace"], w["lnl_trace"], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(d["chain"], w["chain"], rtol=1e-10, atol=1e-12)
        assert d["lnZ"] == pytest.approx(w["lnZ"], rel=1e-9, abs=1e-9) and math.isnan(d["lnZ_se"])
    assert sum(int(w["swap_trace"].sum()) for w in want) > 0


def test_a_stream_gives_the_bits_of_the_default_stream():
    import torch
    stream = torch.cuda.Stream()
    got = _raw_run(_three_regions(), THREE_IDS, stream=stream.cuda_stream)
    stream.synchronize()
    for g, (a, b) in enumerate(zip(_three_host(), got)):
        _assert_same(a, b, ("stream", g))


def test_device_chains_of_three_regions_one_of_them_absent():
    host = _three_host()
    got = _raw_run(_three_regions(), THREE_IDS, device_chain=True, no_chain=(1,))
    assert got[1]["chain"] is None and got[0]["chain"].shape == (5, 6, 3) and got[2]["chain"].shape == (5, 6, 10)
    for g, (a, b) in enumerate(zip(host, got)):
        _assert_same(a, b, ("device chain", g))
    half = _raw_run(_three_regions(), THREE_IDS, no_chain=(1,))          # host chains with the same NULL entry
    for g, (a, b) in enumerate(zip(host, half)):
        _assert_same(a, b, ("host chain, one absent", g))


def test_batch_order_and_a_repeated_region():
    """theta_off / out_off with unequal D: each region, wherever it stands in a batch, has the bits it has alone"""
    regions, host = _three_regions(), _three_host()
    alone = [_raw_run([R], [i])[0] for R, i in zip(regions, THREE_IDS)]
    for g in range(3):
        _assert_same(alone[g], host[g], ("alone", g))
    back = _raw_run(regions[::-1], THREE_IDS[::-1])
    for g in range(3):
        _assert_same(alone[g], back[2 - g], ("reversed", g))
    twice = _raw_run([regions[1], regions[0], regions[1], regions[2]], [3, 11, 77, 40])
    _assert_same(alone[1], twice[0], "repeated, first")
    _assert_same(alone[0], twice[1], "repeated, between")
    _assert_same(alone[2], twice[3], "repeated, last")
    other = _raw_run([regions[1]], [77])[0]
    _assert_same(other, twice[2], "repeated, under its second id")
    assert not np.array_equal(other["chain"], alone[1]["chain"])         # the id keys the draws
