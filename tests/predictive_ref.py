"""Numpy restatement of the pointwise predictive density and WAIC (include/vamp_pred.h, DESIGN.md "Pointwise
predictive density and WAIC"): the yardstick of tests/test_predictive.py and tests/test_gpu_predictive.py.  The
bad-sample rule and the optical depths are posterior_ref's, so the flux is the one the posterior tests hold the device to."""
import numpy as np

import posterior_ref as pref

PIX = ("lppd", "ll_mean", "p_waic_pix")
GRP = ("elpd_waic", "elpd_se", "p_waic", "lnl_mean")
CNT = ("n_high", "n_used", "n_bad")
FLAT = PIX + GRP + CNT
HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)


def bad_samples(theta, K, mode, sample_sd):
    """posterior_ref's rule; with a free sd also an sd that is not finite or <= 0"""
    bad = pref.bad_samples(theta, K, mode)
    if sample_sd:
        with np.errstate(invalid="ignore"):
            bad |= ~np.isfinite(theta[:, -1]) | (theta[:, -1] <= 0)
    return bad


def loglik(x, flux, noise, theta, K, mode, sample_sd):
    """(l[n, P] of the good samples of ``theta`` [S, D], their model flux f[n, P], sigma broadcastable to [n, P], bad[S])"""
    bad = bad_samples(theta, K, mode, sample_sd)
    good = theta[~bad]
    with np.errstate(all="ignore"):
        f = np.exp(-pref.sample_taus(x, good, K, mode).sum(axis=1))
        sigma = good[:, -1][:, None] if sample_sd else np.asarray(noise, dtype=np.float64)[None, :]
        r = (np.asarray(flux, dtype=np.float64)[None, :] - f) / sigma
        ll = -0.5 * r ** 2 - np.log(sigma) - HALF_LN_2PI
    return ll, f, sigma, bad


def column_stats(ll):
    """(lppd, ll_mean, p_waic_pix) [P] of l[n, P] by the header's formulas"""
    n, P = ll.shape
    nan = np.full(P, np.nan)
    if n == 0:
        return nan, nan.copy(), nan.copy()
    with np.errstate(all="ignore"):
        m = np.max(ll, axis=0)
        lppd = m + np.log(np.sum(np.exp(ll - m), axis=0) / n)
        mean = np.sum(ll, axis=0) / n
        pw = np.sum((ll - mean) ** 2, axis=0) / (n - 1) if n > 1 else nan.copy()
    return lppd, mean, pw


def totals(lppd, pw, mean):
    P = lppd.size
    elpd = lppd - pw
    with np.errstate(all="ignore"):
        return {"elpd_waic": float(np.sum(elpd)), "p_waic": float(np.sum(pw)), "lnl_mean": float(np.sum(mean)),
                "elpd_se": float(np.sqrt(P * np.var(elpd, ddof=1))) if P > 1 else float("nan"), "n_high": int(np.sum(pw > 0.4))}


def pointwise(x, flux, noise, chain, K, mode, sample_sd):
    """dict of the header's outputs for one group: chain [N, W, D] (sample s = t W + w); also ``d``, the [P] factor of the
    test bars: max over the good samples of |y - f| / sigma^2"""
    chain = np.asarray(chain, dtype=np.float64)
    theta = chain.reshape(-1, chain.shape[2])
    ll, f, sigma, bad = loglik(x, flux, noise, theta, K, mode, sample_sd)
    lppd, mean, pw = column_stats(ll)
    with np.errstate(all="ignore"):
        d = np.max(np.abs(np.asarray(flux)[None, :] - f) / sigma ** 2, axis=0) if ll.shape[0] else np.zeros(len(x))
    return {"lppd": lppd, "ll_mean": mean, "p_waic_pix": pw, **totals(lppd, pw, mean), "n_used": int((~bad).sum()),
            "n_bad": int(bad.sum()), "d": d}


def flat(records):
    """the library's flat outputs (group order) from per-group dicts: what vamp_amd.predictive._pred_host returns"""
    out = {k: np.concatenate([np.ravel(r[k]) for r in records]) for k in PIX}
    out.update({k: np.array([r[k] for r in records], dtype=np.float64) for k in GRP})
    out.update({k: np.array([r[k] for r in records], dtype=np.int32) for k in CNT})
    return out


def fake_pred_host(calls=None, planted=None):
    """stand-in for vamp_amd.predictive._pred_host: the restatement instead of the library call.  ``planted``: a function
    (group's n_comp) -> per-pixel elpd to plant (lppd = that, p_waic_pix = 0), for the ladder tests"""
    def host(xs, fluxes, noises, arrays, n_comp, modes, steps, device, scratch_bytes):
        if calls is not None:
            calls.append((len(arrays), list(steps)))
        recs = [pointwise(x, y, n, a[::s], k, m, n is None) for x, y, n, a, k, m, s in zip(xs, fluxes, noises, arrays, n_comp, modes, steps)]
        if planted is not None:
            for r, k in zip(recs, n_comp):
                r["lppd"] = np.asarray(planted(k), dtype=np.float64)
                r["p_waic_pix"] = np.zeros_like(r["lppd"])
        return flat(recs)
    return host


def bars(want):
    """the tolerances of the GPU comparison for one group's restatement ``want``, from the flux bar 1e-12 of
    tests/test_gpu_posterior.py: a flux error df moves l by |y - f| / sigma^2 df"""
    d = 1e-12 * want["d"]
    with np.errstate(all="ignore"):
        b = {"lppd": d + 1e-12 * np.maximum(1.0, np.abs(want["lppd"])), "ll_mean": d + 1e-12 * np.maximum(1.0, np.abs(want["ll_mean"])),
             "p_waic_pix": 2.0 * np.sqrt(want["p_waic_pix"]) * d + 1e-12 * np.maximum(1.0, want["p_waic_pix"])}
    fin = lambda v: np.where(np.isfinite(v), v, 0.0)
    b["elpd_waic"] = float(np.sum(fin(b["lppd"]) + fin(b["p_waic_pix"])))
    b["p_waic"] = float(np.sum(fin(b["p_waic_pix"])))
    b["lnl_mean"] = float(np.sum(fin(b["ll_mean"])))
    return b


def same_pattern(got, want):
    """NaN and +-inf in the same places"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
                and np.array_equal(np.isneginf(got), np.isneginf(want)))


def check(got, want, label=""):
    """asserts one group's library result ``got`` (dict of the header's outputs) against its restatement at the bars;
    returns the worst ratio error / bar over the finite values"""
    b = bars(want)
    worst = 0.0
    for k in PIX + ("elpd_waic", "p_waic", "lnl_mean"):
        g, w = np.atleast_1d(np.asarray(got[k], dtype=np.float64)), np.atleast_1d(np.asarray(want[k], dtype=np.float64))
        assert same_pattern(g, w), (label, k, "NaN / inf pattern", g, w)
        fin = np.isfinite(w)
        if fin.any():
            ratio = np.abs(g[fin] - w[fin]) / np.broadcast_to(np.atleast_1d(b[k]), w.shape)[fin]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (label, k, float(ratio.max()))
    g, w = float(got["elpd_se"]), float(want["elpd_se"])
    assert same_pattern(g, w), (label, "elpd_se", g, w)
    if np.isfinite(w):
        rel = abs(g - w) / max(abs(w), np.finfo(float).tiny)
        worst = max(worst, rel / 1e-9)
        assert rel <= 1e-9, (label, "elpd_se", rel)
    for k in CNT:
        assert int(got[k]) == int(want[k]), (label, k, got[k], want[k])
    return worst
