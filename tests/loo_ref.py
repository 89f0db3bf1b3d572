"""Numpy restatement of PSIS-LOO (include/vamp_loo.h, DESIGN.md "PSIS-LOO: leave-one-out predictive density per
pixel"): the yardstick of tests/test_loo.py and tests/test_gpu_loo.py.  The log-likelihood matrix, the bad-sample rule
and lppd are predictive_ref's, so the evaluation is held to what the WAIC tests hold it to.

``psis_column(l, dtype, plant)`` follows the header line by line in ``dtype`` arithmetic (np.float64, or np.longdouble
for the rounding test); ``plant`` switches on one deliberate error for the tests that show the GPU bars would see it."""
import math

import numpy as np

import predictive_ref as pref

PIX = ("elpd_loo_pix", "p_loo_pix", "khat", "lppd")
GRP = ("elpd_loo", "elpd_loo_se", "p_loo")
CNT = ("n_high_k", "n_used", "n_bad")
FLAT = PIX + GRP + CNT
HIGH_KHAT = 0.7
PLANTS = ("M off by one", "prior left out", "no truncation", "cutoff inside the tail")


def tail_len(n):
    """min(ceil(n / 5), smallest m3 with m3^2 >= 9 n), in integers"""
    m3 = math.isqrt(9 * n)
    m3 += m3 * m3 < 9 * n
    return min(-(-n // 5), m3)


def gpdfit(x, T=np.float64, prior=True):
    """Zhang & Stephens' fit of the generalised Pareto distribution to the ascending x, as loo::gpdfit: (khat, sigma)"""
    x = np.asarray(x, dtype=T)
    M = x.size
    m = 30 + math.isqrt(M)
    j = np.arange(1, m + 1, dtype=T)
    xq = x[(M + 2) // 4 - 1]                       # floor(M / 4 + 0.5), 1-based
    with np.errstate(all="ignore"):
        theta = 1 / x[-1] + (1 - np.sqrt(T(m) / (j - T(0.5)))) / (3 * xq)
        kj = np.mean(np.log1p(-theta[:, None] * x[None, :]), axis=1)
        lj = M * (np.log(-theta / kj) - kj - 1)
        w = 1 / np.sum(np.exp(lj[None, :] - lj[:, None]), axis=1)
        theta_hat = np.sum(theta * w)
        k = np.mean(np.log1p(-theta_hat * x))
        sigma = -k / theta_hat
        if prior:
            k = (k * M + 5) / (T(M) + 10)
    return k, sigma


def psis_column(l, dtype=np.float64, plant=None):
    """(elpd_loo, khat) of one pixel's log-likelihood ``l`` over its good samples, in sample order"""
    T = dtype
    l = np.asarray(l, dtype=T)
    n = l.size
    if n == 0 or not np.isfinite(l).all():
        return T(np.nan), T(np.nan)
    r = -l
    r = r - r.max()
    M = tail_len(n) + (plant == "M off by one")
    khat = T(np.inf)
    lw = r.copy()
    if M >= 5:
        order = np.argsort(r, kind="stable")           # ascending by (value, sample index)
        tail = order[n - M:]
        cutoff = r[order[n - M - 1 + (plant == "cutoff inside the tail")]]
        with np.errstate(all="ignore"):
            x = np.exp(r[tail]) - np.exp(cutoff)
            if r[tail[-1]] > r[tail[0]] and x[(M + 2) // 4 - 1] > 0:
                khat, sigma = gpdfit(x, T, prior=plant != "prior left out")
                if np.isfinite(khat):
                    p = (np.arange(1, M + 1, dtype=T) - T(0.5)) / M
                    lw[tail] = np.log(sigma * np.expm1(-khat * np.log1p(-p)) / khat + np.exp(cutoff))
    if plant != "no truncation":
        lw = np.where(lw > 0, T(0), lw)
    with np.errstate(all="ignore"):
        mx = lw.max()
        lw = lw - (mx + np.log(np.sum(np.exp(lw - mx))))
        v = l + lw
        mv = v.max()
        return mv + np.log(np.sum(np.exp(v - mv))), khat


def columns(ll, dtype=np.float64, plant=None):
    """(elpd_loo_pix, khat) [P] of l[n, P]"""
    P = ll.shape[1]
    res = [psis_column(ll[:, p], dtype, plant) for p in range(P)]
    return np.array([r[0] for r in res], dtype=dtype), np.array([r[1] for r in res], dtype=dtype)


def totals(elpd, ploo, khat):
    P = elpd.size
    with np.errstate(all="ignore"):
        return {"elpd_loo": float(np.sum(elpd)), "p_loo": float(np.sum(ploo)),
                "elpd_loo_se": float(np.sqrt(P * np.var(elpd, ddof=1))) if P > 1 else float("nan"), "n_high_k": int(np.sum(khat > HIGH_KHAT))}


def from_loglik(ll, skip=None, plant=None):
    """dict of the header's outputs for one [S, P] matrix; ``skip``: S flags, 1 = leave the sample out"""
    ll = np.asarray(ll, dtype=np.float64)
    bad = np.zeros(ll.shape[0], bool) if skip is None else np.asarray(skip).astype(bool)
    good = ll[~bad]
    lppd = pref.column_stats(good)[0]
    elpd, khat = columns(good, plant=plant)
    with np.errstate(all="ignore"):
        ploo = lppd - elpd
    return {"elpd_loo_pix": elpd, "p_loo_pix": ploo, "khat": khat, "lppd": lppd, **totals(elpd, ploo, khat),
            "n_used": int((~bad).sum()), "n_bad": int(bad.sum())}


def pointwise(x, flux, noise, chain, K, mode, sample_sd):
    """dict of the header's outputs for one group: chain [N, W, D] (sample s = t W + w); also ``ll`` [S, P] (rows of bad
    samples NaN), ``bad`` [S], and predictive_ref.pointwise's ``ll_mean``, ``p_waic_pix`` and ``d`` (for its bars)"""
    chain = np.asarray(chain, dtype=np.float64)
    theta = chain.reshape(-1, chain.shape[2])
    good, f, sigma, bad = pref.loglik(x, flux, noise, theta, K, mode, sample_sd)
    ll = np.full((theta.shape[0], len(x)), np.nan)
    ll[~bad] = good
    out = from_loglik(ll, bad)
    waic = pref.pointwise(x, flux, noise, chain, K, mode, sample_sd)
    with np.errstate(all="ignore"):
        dl = np.abs(np.asarray(flux)[None, :] - f) / sigma ** 2 * np.ones_like(good)
    full = np.zeros_like(ll)
    full[~bad] = dl
    out.update(ll=ll, bad=bad, dl=full, ll_mean=waic["ll_mean"], p_waic_pix=waic["p_waic_pix"], d=waic["d"])
    return out


def flat(records):
    """the library's flat outputs (group order) from per-group dicts: what vamp_amd.loo._loo_host returns"""
    out = {k: np.concatenate([np.ravel(r[k]) for r in records]) for k in PIX}
    out.update({k: np.array([r[k] for r in records], dtype=np.float64) for k in GRP})
    out.update({k: np.array([r[k] for r in records], dtype=np.int32) for k in CNT})
    return out


def fake_loo_host(calls=None, planted=None):
    """stand-in for vamp_amd.loo._loo_host: the restatement instead of the library call.  ``planted``: a function
    (group's n_comp) -> per-pixel elpd_loo to plant, for the ladder tests"""
    def host(xs, fluxes, noises, arrays, n_comp, modes, steps, device, scratch_bytes):
        if calls is not None:
            calls.append((len(arrays), list(steps)))
        recs = [pointwise(x, y, n, a[::s], k, m, n is None) for x, y, n, a, k, m, s in zip(xs, fluxes, noises, arrays, n_comp, modes, steps)]
        if planted is not None:
            for r, k in zip(recs, n_comp):
                r["elpd_loo_pix"] = np.asarray(planted(k), dtype=np.float64)
                r["p_loo_pix"] = r["lppd"] - r["elpd_loo_pix"]
                r.update(totals(r["elpd_loo_pix"], r["p_loo_pix"], r["khat"]))
        return flat(recs)
    return host


def bars(want):
    """the tolerances of the GPU comparison of the column stage on exact inputs, for one group's restatement ``want``:
    khat 1e-10 max(1, |khat|), elpd_loo_pix 1e-11 max(1, |v|), p_loo_pix that plus the same bar on lppd, a group sum the
    sum of its pixels' bars (elpd_loo_se: 1e-9 relative, in ``check``)"""
    fin = lambda v: np.where(np.isfinite(v), v, 0.0)
    with np.errstate(all="ignore"):
        b = {"khat": 1e-10 * np.maximum(1.0, np.abs(fin(want["khat"]))), "elpd_loo_pix": 1e-11 * np.maximum(1.0, np.abs(fin(want["elpd_loo_pix"]))),
             "lppd": 1e-11 * np.maximum(1.0, np.abs(fin(want["lppd"])))}
    b["p_loo_pix"] = b["elpd_loo_pix"] + b["lppd"]
    b["elpd_loo"] = float(np.sum(b["elpd_loo_pix"]))
    b["p_loo"] = float(np.sum(b["p_loo_pix"]))
    return b


def check(got, want, label=""):
    """asserts one group's library result ``got`` (dict of the header's outputs) against its restatement at the bars;
    returns the worst ratio error / bar over the finite values"""
    b = bars(want)
    worst = 0.0
    for k in PIX + ("elpd_loo", "p_loo"):
        g, w = np.atleast_1d(np.asarray(got[k], dtype=np.float64)), np.atleast_1d(np.asarray(want[k], dtype=np.float64))
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        assert pref.same_pattern(g, w), (label, k, "NaN / inf pattern", g, w)
        fin = np.isfinite(w)
        if fin.any():
            ratio = np.abs(g[fin] - w[fin]) / np.broadcast_to(np.atleast_1d(b[k]), w.shape)[fin]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (label, k, float(ratio.max()))
    g, w = float(got["elpd_loo_se"]), float(want["elpd_loo_se"])
    assert pref.same_pattern(g, w), (label, "elpd_loo_se", g, w)
    if np.isfinite(w):
        rel = abs(g - w) / max(abs(w), np.finfo(float).tiny)
        worst = max(worst, rel / 1e-9)
        assert rel <= 1e-9, (label, "elpd_loo_se", rel)
    for k in CNT:
        assert int(got[k]) == int(want[k]), (label, k, got[k], want[k])
    return worst


# ---- the inputs the tests share ----------------------------------------------------------------------------------
DATA = {"K4": ("H1215_r0_K4_m1_sd0", 4, 1), "K2": ("H1215_r0_K2_m0_sd0", 2, 0)}     # golden case, lines, mode

# (seed, samples S, data set, free sd) of the column-stage comparison: the sizes at which the tail length takes another
# path (M < 5 | >= 5 at 20 | 21, the two terms of M around 225 .. 231), one wavefront and one workgroup of samples and
# one more, and the longest column; both data sets, known noise and free sd
COLUMN_CASES = [(44, 20, "K4", False), (44, 21, "K4", True), (44, 64, "K2", False), (44, 65, "K2", True), (44, 129, "K4", True),
                (44, 225, "K2", False), (44, 231, "K4", False), (44, 1024, "K2", True), (44, 1025, "K4", False), (44, 4096, "K4", True),
                (44, 16384, "K4", False), (44, 16384, "K2", True)]


def ball_case(seed, S, data, sample_sd):
    """(x, flux, noise or None, theta [S, D], K, mode): a chain like a converged one, a 1 % ball around the fitted point of
    a golden case (with free sd: around sd = the data's noise level)"""
    import posterior_ref
    from conftest import load_golden
    name, K, mode = DATA[data]
    g = load_golden("lnprob_cases.npz")
    fin = np.isfinite(g[name + "_lnprob"])
    x, flux, noise, th = g[name + "_x"], g[name + "_flux"], g[name + "_noise"], g[name + "_theta"][fin][0]
    centre = np.append(th[:(4 if mode == 1 else 3) * K], float(np.median(noise))) if sample_sd else th
    return x, flux, (None if sample_sd else noise), posterior_ref.ball(np.random.default_rng(seed), centre, S), K, mode


_cache = {}


def column_case(case):
    """(l [S, P], the restatement of vamp_loo_from_loglik on it) of one of COLUMN_CASES, computed once"""
    if case not in _cache:
        seed, S, data, sd = case
        x, flux, noise, theta, K, mode = ball_case(seed, S, data, sd)
        ll, _, _, bad = pref.loglik(x, flux, noise, theta, K, mode, sd)
        assert not bad.any()
        ll.setflags(write=False)
        _cache[case] = (ll, from_loglik(ll))
    return _cache[case]
