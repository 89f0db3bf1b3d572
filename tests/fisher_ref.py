"""numpy + scipy restatement of include/vamp_fisher.h for tests/test_fisher.py and
tests/test_gpu_fisher.py: the Jacobian of the model flux from scipy's wofz and the identity w' = -2 z w + 2i / sqrt(pi),
and the gradient, information matrix, covariance and ln det from a given Jacobian.  Also the bars of the issue."""
import numpy as np
from scipy.special import wofz

SQRT_LN2 = np.sqrt(np.log(2.0))
SQRT_PI = np.sqrt(np.pi)
EPS = 2.0 ** -52


def q_of(mode):
    return 4 if mode == 1 else 3


def line_terms(x, th, mode):
    """(tau [P], dtau / dtheta [P, q]) of one line"""
    x = np.asarray(x, dtype=np.float64)
    if mode == 1:
        A, c, L, G = th
        s = 2.0 * SQRT_LN2 / G
        u, y = (x - c) * s, L * SQRT_LN2 / G
        w = wofz(u + 1j * y)
        K, M = w.real, w.imag
        Ku = -2.0 * (u * K - y * M)
        Ky = 2.0 * (u * M + y * K) - 2.0 / SQRT_PI
        tau = A * y * SQRT_PI * K
        return tau, np.stack([y * SQRT_PI * K, -A * y * SQRT_PI * s * Ku, A * SQRT_PI * (SQRT_LN2 / G) * (K + y * Ky),
                              -(A * SQRT_PI * y / G) * (K + u * Ku + y * Ky)], axis=1)
    A, c, sg = th
    u = (x - c) / sg
    e = np.exp(-0.5 * u * u)
    return A * e, np.stack([e, A * e * u / sg, A * e * u * u / sg], axis=1)


def jacobian(x, theta, n_comp, mode, sample_sd=False):
    """(f [P], J [P, D]) at one point; the free sd's column is 0"""
    q = q_of(mode)
    D = q * n_comp + int(bool(sample_sd))
    tau, dt = np.zeros(len(x)), np.zeros((len(x), D))
    for k in range(n_comp):
        t, d = line_terms(x, theta[q * k:q * k + q], mode)
        tau += t
        dt[:, q * k:q * k + q] = d
    f = np.exp(-tau)
    return f, -f[:, None] * dt


def from_jacobian(J, f, flux, noise, theta, n_comp, mode, with_prior=True):
    """grad, info, cov, logdet, chi2 (and a = J / sigma, rs = r / sigma) from a Jacobian; noise None: free sd = theta[-1]"""
    q, P = q_of(mode), len(f)
    Dl = q * n_comp
    sd = noise is None
    sig = np.full(P, theta[-1]) if sd else np.asarray(noise, dtype=np.float64)
    a = J / sig[:, None]
    rs = (np.asarray(flux) - f) / sig
    grad = a.T @ rs
    info = a.T @ a
    chi2 = float(rs @ rs)
    if with_prior:
        for d in range(0, Dl, q):
            grad[d] += 1.0 / theta[d] - 1.0
            info[d, d] += 1.0 / theta[d] ** 2
    if sd:
        grad[Dl] = chi2 / theta[-1] - P / theta[-1]
        info[Dl, :] = info[:, Dl] = 0.0
        info[Dl, Dl] = 2.0 * P / theta[-1] ** 2
    out = {"grad": grad, "info": info, "chi2": chi2, "a": a, "rs": rs}
    with np.errstate(all="ignore"):
        try:
            out["cov"] = np.linalg.inv(info)
            out["logdet"] = float(np.linalg.slogdet(info)[1])
        except np.linalg.LinAlgError:
            out["cov"], out["logdet"] = np.full_like(info, np.nan), float("nan")
    return out


def scaled(info):
    d = np.sqrt(np.diag(info))
    with np.errstate(all="ignore"):
        return info / np.outer(d, d)


def kappa(info):
    """2-norm condition number of the scaled information (inf when it is singular or not finite)"""
    C = scaled(info)
    if not np.all(np.isfinite(C)):
        return float("inf")
    s = np.linalg.svd(C, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else float("inf")


# ---- the bars (b: the case's bar on J; a, rs: from the fixture's J) ---------------------------------------------
def bar_b(e_id):
    return float(np.clip(2.0 * e_id, 1e-12, 1e-10))


def bar_jac(J, b):
    return b * np.abs(J).max(axis=0)


def bar_grad(a, rs, b):
    P = a.shape[0]
    return b * P * np.abs(a).max(axis=0) * np.abs(rs).max() + 4 * P * EPS * np.sum(np.abs(a * rs[:, None]), axis=0)


def bar_info(a, b):
    P = a.shape[0]
    m = np.abs(a).max(axis=0)
    return (2 * b + 4 * EPS) * P * np.outer(m, m)


def bar_prior(theta, n_comp, mode, D):
    """What the prior's terms add to the bars of grad and of info's diagonal: the issue's bars bound the sums over the
    pixels only, and a result 1 / A - 1 + (sum) or 1 / A^2 + (sum) cannot be closer to its fp64 neighbour than the rounding
    of its own terms: 2 eps (1 / A + 1) and 2 eps / A^2 on the amplitude entries (a line of L = 4e-13 has a data term of
    1e-20 beside a prior term of 0.5)."""
    q = q_of(mode)
    g, i = np.zeros(D), np.zeros(D)
    A = np.abs(np.asarray(theta)[0:q * n_comp:q])
    g[0:q * n_comp:q] = 2 * EPS * (1.0 / A + 1.0)
    i[0:q * n_comp:q] = 2 * EPS / A ** 2
    return g, i


def bar_cov(cov, kap, b, P):
    D = cov.shape[0]
    d = np.sqrt(np.diag(cov))
    return D * kap * (2 * b * P + 8 * D * EPS) * np.outer(d, d)


def bar_logdet(D, kap, b, P):
    return D * kap * (2 * b * P + 8 * D * EPS)


# ---- the fixture ------------------------------------------------------------------------------------------------
def load_cases(path):
    """tests/golden/fisher/fisher_cases.npz (tests/golden/make_fisher_golden.py) as a list of dicts: name, kind ('full': every
    quantity; 'jac': compared on J only; 'flat': a point of status 1), x, flux, noise (None: free sd), theta, K, mode, sd,
    D, P, jac, grad, info, cov, logdet, chi2, kappa, e_id, and -- 'full' only -- grad_noprior, info_noprior"""
    g = np.load(path, allow_pickle=False)
    out = []
    for name, kind, region, m in zip(g["cases"], g["kinds"], g["regions"], g["meta"]):
        name, kind, region = str(name), str(kind), str(region)
        K, mode = int(m[0]), int(m[1])
        x, flux = g[region + "_x"], g[region + "_flux"]
        noise = g[region + "_noise"] if region + "_noise" in g.files else None
        P, D = len(x), q_of(mode) * K + int(noise is None)
        v, T = g[name], D * (D + 1) // 2
        assert v.size == 4 * D + 2 * T + P * D, name

        def full(tri):
            mat = np.zeros((D, D))
            mat[np.tril_indices(D)] = tri
            return mat + np.tril(mat, -1).T

        c = {"name": name, "kind": kind, "x": x, "flux": flux, "noise": noise, "theta": v[:D].copy(), "K": K, "mode": mode,
             "sd": noise is None, "D": D, "P": P, "grad": v[D:2 * D].copy(), "info": full(v[4 * D:4 * D + T]),
             "cov": full(v[4 * D + T:4 * D + 2 * T]), "jac": v[4 * D + 2 * T:].reshape(P, D).copy(), "logdet": float(m[2]),
             "chi2": float(m[3]), "kappa": float(m[4]), "e_id": float(m[5])}
        if kind == "full":
            c["grad_noprior"] = v[2 * D:3 * D].copy()
            c["info_noprior"] = c["info"].copy()
            c["info_noprior"][np.diag_indices(D)] = v[3 * D:4 * D]
        out.append(c)
    return out
