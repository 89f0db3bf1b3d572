"""numpy restatement of the chain diagnostics (DESIGN.md "Chain diagnostics"): the yardstick of
vamp_amd/csrc/chain_diag.hip.  Autocovariance by FFT as emcee 3's ``integrated_time`` computes it, then
the window, split-R-hat and degenerate-case rules of the library.  Test infrastructure: the product never
imports it."""
import numpy as np


def _autocov(y):
    """biased autocovariance sums c(k) = sum_t y_t y_{t+k} along axis 0 (y centred), by FFT"""
    N = y.shape[0]
    n = 1 << int(np.ceil(np.log2(2 * N)))
    f = np.fft.rfft(y, n=n, axis=0)
    return np.fft.irfft(f * np.conj(f), n=n, axis=0)[:N]


def diagnostics(chain, c=5.0):
    """chain [N, W, D] -> (tau, n_eff, r_hat, window, reliable), arrays of length D.  A NaN or +-inf anywhere in the series
    of any walker of a parameter gives tau = n_eff = r_hat = NaN, window = -1 and reliable = False for that parameter alone;
    this comes before "a walker's series is constant" (include/vamp_diag.h)"""
    chain = np.asarray(chain, dtype=np.float64)
    N, W, D = chain.shape
    tau, n_eff, r_hat = np.full(D, np.nan), np.full(D, np.nan), np.full(D, np.nan)
    window, reliable = np.full(D, -1, dtype=np.int32), np.zeros(D, dtype=bool)
    if N < 4:
        return tau, n_eff, r_hat, window, reliable
    n = N // 2
    for d in range(D):
        x = chain[:, :, d]
        if not np.isfinite(x).all():                         # a NaN or an infinity in any walker's series: NaN, window -1,
            continue                                         # not reliable; this comes before "stuck"
        stuck = np.ptp(x, axis=0) == 0                       # c_w(0) = 0: a constant series
        # split-R-hat (BDA3, no rank normalisation); a constant walker's halves have mean x_0 and variance 0
        seq = np.concatenate([x[:n], x[N - n:]], axis=1)     # [n, 2W]
        means = seq.mean(0)
        var = seq.var(0, ddof=1)
        s2 = np.concatenate([stuck, stuck])
        means[s2] = np.concatenate([x[0], x[0]])[s2]
        var[s2] = 0.0
        B = n * np.sum((means - means.mean()) ** 2) / (2 * W - 1)
        V = var.mean()
        if V > 0:
            r_hat[d] = np.sqrt(((n - 1) / n * V + B / n) / V)
        else:
            r_hat[d] = np.inf if B > 0 else np.nan
        if stuck.any():
            tau[d], n_eff[d] = np.inf, 0.0
            continue
        acf = _autocov(x - x.mean(0))
        rho = (acf / acf[0]).mean(1)
        taus = 2.0 * np.cumsum(rho) - 1.0
        ok = np.arange(N) >= c * taus
        found = bool(ok.any())
        M = int(np.argmax(ok)) if found else N - 1
        tau[d], window[d] = taus[M], (M if not np.isnan(taus[M]) else -1)
        n_eff[d] = N * W / taus[M] if taus[M] > 0 else np.nan
        reliable[d] = found and taus[M] > 0 and N >= 50.0 * max(taus[M], 1.0)
    return tau, n_eff, r_hat, window, reliable


def ar1(rng, N, W, D, rho, burn=200):
    """W walkers of D independent AR(1) series x_t = rho x_{t-1} + e_t: tau = (1 + rho) / (1 - rho)"""
    x = np.zeros((N + burn, W, D))
    e = rng.standard_normal((N + burn, W, D))
    for t in range(1, N + burn):
        x[t] = rho * x[t - 1] + e[t]
    return x[burn:]


def two_modes(rng, N, W, D, sep=10.0, rho=0.5):
    """half of the walkers around -sep/2, half around +sep/2: a split ensemble"""
    x = ar1(rng, N, W, D, rho)
    x[:, : W // 2] -= sep / 2
    x[:, W // 2:] += sep / 2
    return x
