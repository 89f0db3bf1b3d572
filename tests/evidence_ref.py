"""numpy restatement of libvamp_evid.so (include/vamp_evid.h, DESIGN.md "Evidence"): the same ladder, the same draws,
the same swaps and the same reductions, built on the oracle's log_like, log_prior, philox4x32_10, draw_move_batch and
split_tables_batch.  Slow and plain: the GPU tests compare trajectories of a few steps against it, the CPU tests use
its pieces."""
import math

import numpy as np

from oracle import vamp_oracle as vo

STREAM_SWAP, STREAM_PRIOR = 3, 4
N_BLOCKS = 8
_M = vo.MASK32


def default_betas(T):
    """the ladder of vamp_evid_default_betas through the C library's pow, as the library takes it: numpy's array power is
    an ulp off it in places (first at T = 33), and a ladder an ulp off is another trajectory"""
    b = np.array([math.pow(j / (T - 1.0), 1.0 / 0.3) for j in range(T)])
    b[0], b[-1] = 0.0, 1.0
    return b


def make_region(x, flux, noise, n_comp, mode, sample_sd=False, bounds=None):
    """the oracle's Region with the library's bounds: given, or derived from x in either direction"""
    x = np.asarray(x, dtype=np.float64)
    if bounds is None:
        lo, hi = min(x[0], x[-1]), max(x[0], x[-1])
        smax = (hi - lo) / 2.0
        bounds = (lo, hi, smax, smax * 2 * np.sqrt(2 * np.log(2.0)))
    noise = np.ones_like(x) if noise is None else noise
    return vo.Region(x, flux, noise, int(n_comp), mode=int(mode), sample_sd=bool(sample_sd), include_norm=True, c_lo=float(bounds[0]),
                     c_hi=float(bounds[1]), sigma_max=float(bounds[2]), fwhm_max=float(bounds[3]))


def lnlike_lnprior(region, theta):
    """(ln L, ln pi) of one parameter vector: outside the prior (-inf) ln L is NaN, not evaluated; a ln L that is not
    finite is -inf.  A width of exactly 0 lies inside the oracle's prior ([0, max]) and its ln L does not exist (G_fwhm = 0
    divides by zero in Python floats, sigma = 0 on a pixel gives 0 / 0): -inf as well"""
    theta = np.asarray(theta, dtype=np.float64)
    lp = vo.log_prior(region, theta)
    if not lp > -np.inf:
        return np.nan, -np.inf
    try:
        ll = vo.log_like(region, theta)
    except ZeroDivisionError:
        ll = np.nan
    return (ll if np.isfinite(ll) else -np.inf), lp


def lnlike_batch(region, thetas):
    out = np.array([lnlike_lnprior(region, t) for t in np.asarray(thetas, dtype=np.float64)]).reshape(-1, 2)
    return out[:, 0], out[:, 1]


def target(lp, ll, beta):
    """ln of the tempered target pi L^beta; -inf outside the prior or without a finite ln L"""
    lp, ll = np.asarray(lp, dtype=np.float64), np.asarray(ll, dtype=np.float64)
    ok = (lp > -np.inf) & np.isfinite(ll)
    with np.errstate(invalid="ignore"):
        return np.where(ok, lp + beta * np.where(ok, ll, 0.0), -np.inf)


def prior_draws(region, rid, W, seed):
    """W prior draws of sampler region id ``rid`` = region_id * T + j: counter {gid lo, d, STREAM_PRIOR, gid hi}"""
    key = (seed & _M, (seed >> 32) & _M)
    q, D = region.q, region.ndim
    w_max = region.sigma_max if region.mode == vo.MODE_GAUSS3 else region.fwhm_max
    X = np.empty((W, D))
    for w in range(W):
        gid = rid * W + w
        for d in range(D):
            r = vo.philox4x32_10((gid & _M, d, STREAM_PRIOR, (gid >> 32) & _M), key)
            u0 = vo._u53(r[0], r[1])
            u1, u2 = 1.0 - u0, 1.0 - vo._u53(r[2], r[3])
            if region.sample_sd and d == D - 1:
                X[w, d] = u1
            elif d % q == 0:
                X[w, d] = -math.log(u1) - math.log(u2)
            elif d % q == 1:
                X[w, d] = region.c_lo + (region.c_hi - region.c_lo) * u0
            else:
                X[w, d] = w_max * u1
    return X


def swap_rule(ll_lo, ll_hi, dbeta, logu):
    """exchange walker w of rungs j and j + 1 when log u < (beta_{j+1} - beta_j)(ln L_j - ln L_{j+1})"""
    with np.errstate(invalid="ignore"):
        return logu < dbeta * (np.asarray(ll_lo) - np.asarray(ll_hi))


def swap_logu(seed, n, region_id, j, W):
    key = (seed & _M, (seed >> 32) & _M)
    out = np.empty(W)
    for w in range(W):
        r = vo.philox4x32_10((region_id, n, (j << 8) | STREAM_SWAP, w), key)
        u = vo._u53(r[0], r[1])
        out[w] = math.log(u) if u > 0 else -np.inf
    return out


def _stretch_step(region, X, ll, lp, beta, seed, step, rid, a):
    """one full step of one rung, in place; returns the number of accepted moves"""
    W, D = X.shape
    red, blue = vo.split_tables_batch(seed, step, W, W, rid)
    nacc = 0
    for half in (0, 1):
        act, comp = (red, blue) if half == 0 else (blue, red)
        zz, jj, logu = vo.draw_move_batch(seed, step, half, act + rid * W, W // 2, a)
        Xc, Xs = X[comp[jj]], X[act]
        prop = Xc - (Xc - Xs) * zz[:, None]
        ll_q, lp_q = lnlike_batch(region, prop)
        with np.errstate(invalid="ignore"):
            diff = (D - 1.0) * np.log(zz) + target(lp_q, ll_q, beta) - target(lp[act], ll[act], beta)
            acc = logu < diff
        X[act[acc]], ll[act[acc]], lp[act[acc]] = prop[acc], ll_q[acc], lp_q[acc]
        nacc += int(acc.sum())
    return nacc


def log_mean_exp(v):
    v = np.asarray(v, dtype=np.float64).ravel()
    m = v.max()
    return m + math.log(np.mean(np.exp(v - m)))


def stepping_stone(trace, betas):
    """trace [n, T, W] -> sum over j < T - 1 of log mean exp((beta_{j+1} - beta_j) ln L of rung j)"""
    return sum(log_mean_exp((betas[j + 1] - betas[j]) * trace[:, j]) for j in range(len(betas) - 1))


def block_borders(n):
    """the borders of the 8 time blocks of n kept steps: block b is the kept steps borders[b] .. borders[b + 1] - 1"""
    return [b * n // N_BLOCKS for b in range(N_BLOCKS + 1)]


def reduce(trace, betas, borders=None):
    """the reductions of k_evid_reduce from the kept ln L [n_keep, T, W]; ``zb``: the block estimates behind ``lnZ_se``
    (None with fewer than 8 kept steps).  ``borders``: other block borders than the library's (the controls of the tests)"""
    n = trace.shape[0]
    mean, var = trace.mean(axis=(0, 2)), trace.var(axis=(0, 2))
    se, zb = np.nan, None
    if n >= N_BLOCKS:
        bd = block_borders(n) if borders is None else list(borders)
        zb = np.array([stepping_stone(trace[bd[b]:bd[b + 1]], betas) for b in range(N_BLOCKS)])
        se = float(np.std(zb, ddof=1) / math.sqrt(N_BLOCKS))
    ti = float(np.sum(np.diff(betas) * 0.5 * (mean[:-1] + mean[1:])))
    return {"lnZ": stepping_stone(trace, betas), "lnZ_se": se, "lnZ_ti": ti, "mean_lnL": mean, "var_lnL": var, "zb": zb}


def run(regions, region_ids, betas, W, n_steps, burn, swap_every, seed, a=2.0, starts=None):
    """the whole call for a list of oracle Regions; per region a dict with the outputs of vamp_evid_run"""
    betas = np.asarray(betas, dtype=np.float64)
    T = betas.size
    n_keep, n_swaps = n_steps - burn, (n_steps - 1) // swap_every
    out = []
    for g, (R, rid0) in enumerate(zip(regions, region_ids)):
        D = R.ndim
        X = np.empty((T, W, D))
        for j in range(T):
            X[j] = starts[g] if starts is not None and starts[g] is not None else prior_draws(R, rid0 * T + j, W, seed)
        ll, lp = np.empty((T, W)), np.empty((T, W))
        for j in range(T):
            ll[j], lp[j] = lnlike_batch(R, X[j])
        assert np.all(lp > -np.inf) and np.all(np.isfinite(ll)), "a start point is outside the prior or has no finite ln L"
        trace, chain, chain_ll = np.empty((n_keep, T, W)), np.empty((n_keep, W, D)), np.empty((n_keep, W))
        swaps = np.zeros((n_swaps, T - 1, W), dtype=np.uint8)
        nacc, nswap, n = np.zeros(T), np.zeros(T - 1), 0
        for step in range(n_steps):
            for j in range(T):
                nacc[j] += _stretch_step(R, X[j], ll[j], lp[j], betas[j], seed, step, rid0 * T + j, a)
            if step >= burn:
                trace[step - burn], chain[step - burn], chain_ll[step - burn] = ll, X[T - 1], ll[T - 1]
            if (step + 1) % swap_every == 0 and n < n_swaps:
                for j in range(n % 2, T - 1, 2):
                    yes = swap_rule(ll[j], ll[j + 1], betas[j + 1] - betas[j], swap_logu(seed, n, rid0, j, W))
                    swaps[n, j] = yes
                    for arr in (X, ll, lp):
                        lo = arr[j, yes].copy()
                        arr[j, yes] = arr[j + 1, yes]
                        arr[j + 1, yes] = lo
                    nswap[j] += yes.sum()
                n += 1
        rec = reduce(trace, betas)
        offered = np.array([(n_swaps + 1) // 2 if j % 2 == 0 else n_swaps // 2 for j in range(T - 1)], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            rec.update(move_accept=nacc / (n_steps * W), swap_accept=np.where(offered > 0, nswap / (offered * W), np.nan), chain=chain,
                       chain_lnl=chain_ll, lnl_trace=trace, swap_trace=swaps, betas=betas)
        out.append(rec)
    return out


def gauss_line_data(n_pix, lines, noise, seed):
    """the test data of the issue: x = 0 .. n_pix - 1, flux = exp(-sum of Gaussian lines (A, c, sigma)) + noise * N(0, 1)
    from numpy's default_rng(seed)"""
    x = np.arange(float(n_pix))
    tau = sum(vo.gauss_function(x, A, c, s) for A, c, s in lines)
    return x, np.exp(-tau) + noise * np.random.default_rng(seed).standard_normal(n_pix), np.full(n_pix, float(noise))


def quadrature_lnZ(x, flux, noise, n, a_max=12.0):
    """brute-force ln Z of ONE Gaussian line: the midpoint rule on n^3 points over A in [0, a_max] (the prior mass
    beyond is 13 e^-12), c and sigma over their prior ranges"""
    R = make_region(x, flux, noise, 1, vo.MODE_GAUSS3)
    A = (np.arange(n) + 0.5) * (a_max / n)
    c = R.c_lo + (np.arange(n) + 0.5) * ((R.c_hi - R.c_lo) / n)
    s = (np.arange(n) + 0.5) * (R.sigma_max / n)
    lp = (np.log(A) - A)[:, None, None] - math.log(R.c_hi - R.c_lo) - math.log(R.sigma_max)
    prof = np.exp(-0.5 * ((x[None, None, :] - c[:, None, None]) / s[None, :, None]) ** 2)          # [c, s, P]
    ll = np.empty((n, n, n))
    for i, amp in enumerate(A):
        ll[i] = -0.5 * np.sum(((flux - np.exp(-amp * prof)) / noise) ** 2, axis=2)
    ll += R.norm_const
    v = (lp + ll).ravel()
    m = v.max()
    return m + math.log(np.sum(np.exp(v - m))) + math.log((a_max / n) * ((R.c_hi - R.c_lo) / n) * (R.sigma_max / n))


class FakeLibrary:
    """stands in for ``vamp_amd.evidence._run`` in the wiring tests: counts the calls and answers with the restatement's
    reductions of a cheap made-up trace (no sampling)"""

    def __init__(self):
        self.calls = []

    def __call__(self, specs, betas, walkers, steps, burn, swap_every, seed, a, starts, device, want_chain, want_trace=False):
        self.calls.append(len(specs))
        betas = np.asarray(betas)
        out = []
        for g, sp in enumerate(specs):
            rng = np.random.default_rng(1000 + int(sp["region_id"]) + 17 * int(sp["n_comp"]))
            D = (4 if sp["mode"] == 1 else 3) * sp["n_comp"] + int(bool(sp["sample_sd"]))
            # two lines fit the fake data best: ln L rises with beta, most for K = 2
            trace = -5.0 * abs(sp["n_comp"] - 2) - 3.0 * (1 - betas)[None, :, None] + 0.01 * rng.standard_normal((steps - burn, betas.size, walkers))
            rec = reduce(trace, betas)
            rec.update(betas=betas.copy(), move_accept=np.full(betas.size, 0.5), swap_accept=np.full(betas.size - 1, 0.5))
            if want_chain:
                rec.update(chain=rng.random((steps - burn, walkers, D)), chain_lnl=trace[:, -1].copy())
            out.append(rec)
        return out
