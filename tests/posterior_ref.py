"""Numpy restatement of the posterior summaries (include/vamp_post.h, DESIGN.md "Posterior summaries"): the
yardstick of tests/test_posterior.py and tests/test_gpu_posterior.py.  Built on the oracle's profile functions,
np.mean, np.std and np.quantile."""
import numpy as np

from oracle import vamp_oracle as vo

FLAT = ("flux_mean", "flux_sd", "flux_q", "ew_mean", "ew_sd", "ew_q", "comp_ew_mean", "comp_ew_sd", "comp_ew_q", "n_used", "n_bad")


def bad_samples(theta, K, mode):
    """[S] bool: a parameter of the q K that is not finite, or sigma <= 0, or G_fwhm <= 0, or L_fwhm < 0"""
    q = 4 if mode == vo.MODE_VOIGT4 else 3
    t = theta[:, :q * K].reshape(-1, K, q)
    bad = ~np.isfinite(t).all(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        if mode == vo.MODE_VOIGT4:
            bad |= (t[:, :, 3] <= 0).any(axis=1) | (t[:, :, 2] < 0).any(axis=1)
        else:
            bad |= (t[:, :, 2] <= 0).any(axis=1)
    return bad


def sample_taus(x, theta, K, mode):
    """tau[S, K, P] of the good samples ``theta`` [S, D]"""
    q = 4 if mode == vo.MODE_VOIGT4 else 3
    t = theta[:, :q * K].reshape(-1, K, q)[:, :, :, None]
    xx = np.asarray(x, dtype=np.float64)[None, None, :]
    if mode == vo.MODE_VOIGT4:
        return vo.voigt_function(xx, t[:, :, 1], t[:, :, 0], t[:, :, 2], t[:, :, 3])
    return vo.gauss_function(xx, t[:, :, 0], t[:, :, 1], t[:, :, 2])


def _stats(v, probs):
    """mean, population sd and quantiles along axis 0; NaN when there is nothing"""
    if v.shape[0] == 0:
        nan = np.full(v.shape[1:], np.nan)
        return nan, nan.copy(), np.full((len(probs),) + v.shape[1:], np.nan)
    return np.mean(v, axis=0), np.std(v, axis=0), np.quantile(v, probs, axis=0)


def summaries(x, chain, K, mode, sample_sd=False, probs=(0.025, 0.16, 0.5, 0.84, 0.975), pixel_width=1.0):
    """dict of the header's outputs for one group: chain [N, W, D] (sample s = t W + w)"""
    chain = np.asarray(chain, dtype=np.float64)
    theta = chain.reshape(-1, chain.shape[2])
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    bad = bad_samples(theta, K, mode)
    tau = sample_taus(x, theta[~bad], K, mode)                 # [n, K, P]
    flux = np.exp(-tau.sum(axis=1))                            # [n, P]
    ew = np.sum(1.0 - flux, axis=1) * pixel_width              # [n]
    cew = np.sum(1.0 - np.exp(-tau), axis=2) * pixel_width     # [n, K]
    fm, fs, fq = _stats(flux, probs)
    em, es, eq = _stats(ew, probs)
    cm, cs, cq = _stats(cew, probs)
    return {"flux_mean": fm, "flux_sd": fs, "flux_q": fq, "ew_mean": float(em), "ew_sd": float(es), "ew_q": eq,
            "comp_ew_mean": cm, "comp_ew_sd": cs, "comp_ew_q": cq.T.copy(), "n_used": int((~bad).sum()), "n_bad": int(bad.sum())}


def flat(records):
    """the library's flat outputs (group order) from per-group dicts: what vamp_amd.posterior._post_host returns"""
    cat = lambda k: np.concatenate([np.ravel(r[k]) for r in records])
    out = {k: cat(k) for k in ("flux_mean", "flux_sd", "flux_q", "comp_ew_mean", "comp_ew_sd")}
    out["ew_mean"] = np.array([r["ew_mean"] for r in records])
    out["ew_sd"] = np.array([r["ew_sd"] for r in records])
    out["ew_q"] = np.stack([r["ew_q"] for r in records])
    out["comp_ew_q"] = np.concatenate([r["comp_ew_q"] for r in records], axis=0)
    out["n_used"] = np.array([r["n_used"] for r in records], dtype=np.int32)
    out["n_bad"] = np.array([r["n_bad"] for r in records], dtype=np.int32)
    return out


def fake_post_host(calls=None):
    """stand-in for vamp_amd.posterior._post_host: the restatement instead of the library call"""
    def host(xs, arrays, n_comp, modes, sample_sd, widths, probs, steps, device, scratch_bytes):
        if calls is not None:
            calls.append(len(arrays))
        return flat([summaries(x, a[::s], k, m, bool(sd), probs, w)
                     for x, a, k, m, sd, w, s in zip(xs, arrays, n_comp, modes, sample_sd, widths, steps)])
    return host


def draw_prior(rng, x, K, mode, S, sample_sd=False):
    """[S, D] by VPfit._draw_prior's rule: A ~ x e^-x, c ~ U(x0, x1), widths ~ U(0, wmax)"""
    q = 4 if mode == vo.MODE_VOIGT4 else 3
    x0, x1 = min(x[0], x[-1]), max(x[0], x[-1])
    wmax = (x1 - x0) / 2.0 * (vo.FWHM_PER_SIGMA if mode == vo.MODE_VOIGT4 else 1.0)
    th = np.empty((S, q * K + int(sample_sd)))
    for k in range(K):
        o = q * k
        th[:, o] = rng.gamma(2.0, 1.0, S)
        th[:, o + 1] = rng.uniform(x0, x1, S)
        for j in range(2, q):
            th[:, o + j] = rng.uniform(0, wmax, S)
    if sample_sd:
        th[:, -1] = rng.uniform(0, 1, S)
    return th


def ball(rng, theta, S, rel=0.01):
    """[S, D]: a 1 % ball around theta -- what a chain looks like"""
    theta = np.asarray(theta, dtype=np.float64)
    return theta * (1.0 + rel * rng.standard_normal((S, theta.size)))
