"""Numpy restatement of Laplace importance sampling (include/vamp_laplace.h): the yardstick of
tests/test_laplace.py and tests/test_gpu_laplace.py, written once for both.  The draws are the oracle's Philox, the
target is evidence_ref.lnlike_lnprior (the oracle's log_prior and log_like), the weights extend loo_ref's column stage
to -inf entries with its tail length and its generalised Pareto fit, the moments are summed in np.longdouble.

``run(case, plant=None)`` is the whole call for one group; ``plant`` switches on one deliberate error.  ``check(got, case)``
holds a result -- the library's, or a planted restatement's -- to the restatement evaluated on the result's OWN
intermediate outputs, stage by stage, so that each stage answers for its own arithmetic only:

    z          against the restated draws                        32 eps max(1, rho)
    theta      against centre + C z_got                          (D + 2) eps sum_e |C_de z_e| + eps |centre_d|
    lnq        from z_got                                        (D + 4) eps (sum z^2 / 2 + sum |ln C_dd| + (D / 2) ln 2 pi)
    lnp        at theta_got against the oracle                   1e-9 max(1, |value|), identical -inf pattern
    khat, lw   from r = lnp_got - lnq_got                        1e-10 max(1, |khat|), 1e-11 max(1, |lw|)  (loo_ref.bars)
    lnZ ..cov  from lw_got, r and theta_got                      (S + 2) eps sum |terms|, to first order (``_moment_bars``)

The bar on z: u1, u2 and log, sqrt, cos, sin are each good to an ulp or two, and the rounding of 2 pi u2 alone moves z by up
to 2 pi eps rho.  The last stage's restatement forms r - r_max in fp64 exactly as the library does (one rounding, the
same on both sides) and sums in longdouble, so what is left is the library's exp (an ulp per term), its products and
its S additions per sum: (S + 2) eps sum |terms| bounds them, and an output that is a function of several sums gets the
first-order propagation of those bounds."""
import math

import numpy as np

import evidence_ref
import loo_ref
from oracle import vamp_oracle as vo

STREAM_NORMAL = 5
EPS = 2.0 ** -52
Z_BAR_ULPS = 32.0
PLANTS = ("ln det left out of ln q", "rejected draws dropped from the 1 / S", "M off by one", "raw weights in the moments",
          "the sine for both z")
STAGES = ("z", "theta", "lnq", "lnp", "khat", "lw", "lnZ", "lnZ_psis", "lnZ_se", "ess", "mean", "sd", "cov")
_M = vo.MASK32
LD = np.longdouble


def make_case(x, flux, noise, n_comp, mode, centre, chol, n_samples, seed, region_id=0, bounds=None):
    """one group of a call; ``noise`` None = free sd"""
    return {"x": np.asarray(x, dtype=np.float64), "flux": np.asarray(flux, dtype=np.float64),
            "noise": None if noise is None else np.asarray(noise, dtype=np.float64), "n_comp": int(n_comp), "mode": int(mode),
            "sample_sd": noise is None, "centre": np.asarray(centre, dtype=np.float64), "chol": np.asarray(chol, dtype=np.float64),
            "S": int(n_samples), "seed": int(seed), "region_id": int(region_id), "bounds": None if bounds is None else tuple(bounds)}


def region_of(case):
    return evidence_ref.make_region(case["x"], case["flux"], case["noise"], case["n_comp"], case["mode"], case["sample_sd"], case["bounds"])


def draws(S, D, region_id, seed, plant=None):
    """(z [S, D], rho [S, D]): counter {s, j, STREAM_NORMAL, region_id}, key (seed lo, seed hi), through the oracle's
    vectorised Philox (tests/test_oracle.py pins it to philox4x32_10; tests/test_laplace.py pins these draws to it)"""
    npair = (D + 1) // 2
    s, j = np.meshgrid(np.arange(S, dtype=np.uint64), np.arange(npair, dtype=np.uint64), indexing="ij")
    c0, c1, c2, c3 = vo._philox_vec(s, j, STREAM_NORMAL, region_id, seed & _M, (seed >> 32) & _M)
    u53 = lambda hi, lo: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    u1, u2 = 1.0 - u53(c0, c1), u53(c2, c3)
    rho = np.sqrt(-2.0 * np.log(u1))
    a = (2.0 * np.pi) * u2
    first = np.sin(a) if plant == "the sine for both z" else np.cos(a)
    z = np.stack([rho * first, rho * np.sin(a)], axis=2).reshape(S, 2 * npair)[:, :D]
    return np.ascontiguousarray(z), np.repeat(rho, 2, axis=1)[:, :D]


def transform(centre, chol, z):
    """theta [S, D] = centre + tril(C) z in longdouble, and per entry sum_e |C_de z_e|"""
    C = np.tril(np.asarray(chol, dtype=LD))
    zl = np.asarray(z, dtype=LD)
    return np.asarray(centre, dtype=LD) + zl @ C.T, np.abs(zl) @ np.abs(C).T


def ln_q(chol, z, plant=None):
    """(ln q [S], the size of its terms [S]) in longdouble"""
    D = z.shape[1]
    diag = np.log(np.diag(np.asarray(chol, dtype=LD)))
    half = 0.5 * np.sum(np.asarray(z, dtype=LD) ** 2, axis=1)
    const = LD(0.5 * D) * np.log(2 * LD(np.pi))
    ldet = LD(0) if plant == "ln det left out of ln q" else np.sum(diag)
    return -half - ldet - const, half + np.sum(np.abs(diag)) + const


def target(case, theta):
    """ln p [S] of the rows of theta: ln pi + ln L, or -inf for a rejected point"""
    R = region_of(case)
    out = np.empty(len(theta))
    for i, t in enumerate(np.asarray(theta, dtype=np.float64)):
        ll, lp = evidence_ref.lnlike_lnprior(R, t)
        out[i] = lp + ll if lp > -np.inf and np.isfinite(ll) else -np.inf
    return out


def psis_weights(r, dtype=np.float64, plant=None):
    """(lw [S]: the truncated log weights before normalisation, khat, r_max) of the log ratios r, -inf entries allowed:
    loo_ref.psis_column's steps on r in place of -l with n = S; fewer than M + 1 finite values: the raw ratios stand"""
    T = dtype
    r = np.asarray(r, dtype=T)
    n = r.size
    fin = np.isfinite(r)
    rmax = r[fin].max()
    lw = r - rmax
    M = loo_ref.tail_len(n) + (plant == "M off by one")
    khat = T(np.inf)
    if M >= 5 and fin.sum() >= M + 1:
        order = np.argsort(lw, kind="stable")           # ascending by (value, sample index); -inf first
        tail = order[n - M:]
        cutoff = lw[order[n - M - 1]]
        with np.errstate(all="ignore"):
            x = np.exp(lw[tail]) - np.exp(cutoff)
            if lw[tail[-1]] > lw[tail[0]] and x[(M + 2) // 4 - 1] > 0:
                khat, sigma = loo_ref.gpdfit(x, T)
                if np.isfinite(khat):
                    p = (np.arange(1, M + 1, dtype=T) - T(0.5)) / M
                    lw = lw.copy()
                    lw[tail] = np.log(sigma * np.expm1(-khat * np.log1p(-p)) / khat + np.exp(cutoff))
    return np.where(lw > 0, T(0), lw), khat, rmax


def summaries(r, lw, theta, plant=None):
    """the per-group outputs from the log ratios r [S] (fp64, -inf for a rejected draw, at least one finite), the
    truncated log weights lw [S] and the draws theta [S, D]; sums in longdouble.  Also ``terms``: what ``_moment_bars`` needs"""
    r, lw64 = np.asarray(r, dtype=np.float64), np.asarray(lw, dtype=np.float64)
    S = r.size
    fin = np.isfinite(r)
    rmax = r[fin].max()
    with np.errstate(all="ignore"):
        w = np.exp((r - rmax).astype(LD))                # (r - r_max in fp64: the library's one rounding)
        e = np.exp(lw64.astype(LD))
    n = int(fin.sum()) if plant == "rejected draws dropped from the 1 / S" else S
    mean_w = w.sum() / n
    dw = w - mean_w
    var_w = np.sum(dw * dw) / (S - 1)
    wn = e / e.sum()
    wm = w / w.sum() if plant == "raw weights in the moments" else wn
    th = np.asarray(theta, dtype=LD)
    mean = wm @ th
    dev = th - mean
    cov = (dev * wm[:, None]).T @ dev
    out = {"lnZ": rmax + np.log(mean_w), "lnZ_se": np.sqrt(var_w / S) / mean_w, "lnZ_psis": rmax + np.log(e.sum() / S),
           "ess": 1 / np.sum(wn * wn), "mean": mean, "cov": cov, "sd": np.sqrt(np.diag(cov)), "n_out": S - int(fin.sum())}
    out["terms"] = {"rmax": rmax, "mean_w": mean_w, "dw": dw, "wn": wm, "dev": dev, "th": th}
    return out


def _moment_bars(o, S):
    """the bars of the last stage for the restatement ``o`` of ``summaries``: b = (S + 2) eps is the relative bound of one
    sum of S positive terms; a weight w~ = e / sum e carries b + 2 eps, a sum over weighted terms that much more"""
    t = o["terms"]
    b = (S + 2) * EPS
    f = lambda v: float(np.abs(v))
    bars = {"lnZ": b + 4 * EPS * max(1.0, f(t["rmax"]), f(o["lnZ"])), "lnZ_psis": b + 4 * EPS * max(1.0, f(t["rmax"]), f(o["lnZ_psis"]))}
    # var = sum dw^2 / (S - 1) with dw = w - mean: b on the sum, and the mean's own b through 2 |dw| mean_w
    ss = float(np.sum(t["dw"] ** 2))
    rel_var = b * (1.0 + 2.0 * float(t["mean_w"]) * float(np.sum(np.abs(t["dw"]))) / ss) + 4 * EPS if ss > 0 else np.inf
    bars["lnZ_se"] = f(o["lnZ_se"]) * (0.5 * rel_var + b + 4 * EPS)
    bars["ess"] = f(o["ess"]) * (3 * b + 8 * EPS)
    wn, dev, th = t["wn"], np.abs(t["dev"]), t["th"]
    bw = 2 * b + 4 * EPS                                 # a weighted sum: the weight's b + 2 eps, the sum's own b, the product
    bars["mean"] = np.asarray(bw * (wn @ np.abs(th)), dtype=np.float64)
    wdev = wn @ dev                                      # sum w~ |theta_d - mean_d|
    bars["cov"] = np.asarray((bw + 4 * EPS) * ((dev * wn[:, None]).T @ dev), dtype=np.float64) \
        + np.outer(bars["mean"], np.asarray(wdev, dtype=np.float64)) + np.outer(np.asarray(wdev, dtype=np.float64), bars["mean"])
    sd = np.asarray(o["sd"], dtype=np.float64)
    with np.errstate(all="ignore"):
        bars["sd"] = np.where(sd > 0, np.diag(bars["cov"]) / (2 * sd), np.sqrt(np.diag(bars["cov"]))) + 2 * EPS * sd
    return bars


def run(case, plant=None):
    """the whole call for one group: a dict with the library's outputs (include/vamp_laplace.h), fp64"""
    D, S = case["centre"].size, case["S"]
    C, centre = case["chol"], case["centre"]
    nan_vec, nan_s = np.full(D, np.nan), np.full(S, np.nan)
    nothing = {"lnZ": np.nan, "lnZ_se": np.nan, "lnZ_psis": np.nan, "khat": np.nan, "ess": np.nan, "n_out": 0, "mean": nan_vec, "sd": nan_vec,
               "cov": np.full((D, D), np.nan), "lw": nan_s}
    low = np.tril(C)
    if not (np.isfinite(low).all() and np.all(np.diag(C) > 0) and np.isfinite(centre).all()):
        return dict(nothing, status=1, lnp_centre=np.nan, z=np.full((S, D), np.nan), theta=np.full((S, D), np.nan), lnp=nan_s, lnq=nan_s)
    z, _ = draws(S, D, case["region_id"], case["seed"], plant)
    theta = np.asarray(transform(centre, C, z)[0], dtype=np.float64)
    lnq = np.asarray(ln_q(C, z, plant)[0], dtype=np.float64)
    lnp = target(case, theta)
    lnp_centre = float(target(case, centre[None, :])[0])
    per_sample = {"z": z, "theta": theta, "lnp": lnp, "lnq": lnq, "lnp_centre": lnp_centre}
    if not lnp_centre > -np.inf:
        return dict(nothing, status=2, **per_sample)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(lnp), lnp - lnq, -np.inf)
    if not np.isfinite(r).any():
        return dict(nothing, status=0, lnZ=-np.inf, n_out=S, **per_sample)
    lw, khat, _ = psis_weights(r, plant=plant)
    o = summaries(r, lw, theta, plant)
    out = {k: float(o[k]) for k in ("lnZ", "lnZ_se", "lnZ_psis", "ess")}
    out.update({k: np.asarray(o[k], dtype=np.float64) for k in ("mean", "sd", "cov")}, khat=float(khat), lw=lw, n_out=o["n_out"], status=0, **per_sample)
    return out


def _ratio(err, bar):
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    with np.errstate(all="ignore"):
        return float(np.max(np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf)), initial=0.0))


def same_pattern(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) \
        and np.array_equal(np.isneginf(a), np.isneginf(b))


def check(got, case, label="", z_bar_ulps=Z_BAR_ULPS):
    """asserts one group's result ``got`` (dict of the header's outputs, the per-sample ones included) against the
    restatement on its own intermediate outputs; returns the worst error / bar per stage (dict).  Each assertion's
    message opens with the stage's name."""
    D, S = case["centre"].size, case["S"]
    C, centre = case["chol"], case["centre"]
    want_status = run(dict(case, S=2))["status"] if got["status"] != 0 else 0        # (statuses 1 and 2 do not depend on the draws)
    worst = {}
    if got["status"] == 1 or want_status == 1:
        assert got["status"] == want_status, (label, "status", got["status"], want_status)
        for k in ("lnZ", "lnZ_se", "lnZ_psis", "khat", "ess", "lnp_centre", "mean", "sd", "cov", "z", "theta", "lnp", "lnq", "lw"):
            assert np.all(np.isnan(got[k])), (label, "status 1", k)
        assert got["n_out"] == 0, (label, "status 1", "n_out")
        return worst
    z_ref, rho = draws(S, D, case["region_id"], case["seed"])
    worst["z"] = _ratio(np.abs(got["z"] - z_ref), z_bar_ulps * EPS * np.maximum(1.0, rho))
    assert worst["z"] <= 1.0, (label, "z", worst["z"])
    th_ref, size = transform(centre, C, got["z"])
    worst["theta"] = _ratio(np.abs(got["theta"] - th_ref), (D + 2) * EPS * size + EPS * np.abs(centre))
    assert worst["theta"] <= 1.0, (label, "theta", worst["theta"])
    q_ref, size = ln_q(C, got["z"])
    worst["lnq"] = _ratio(np.abs(got["lnq"] - q_ref), (D + 4) * EPS * size)
    assert worst["lnq"] <= 1.0, (label, "lnq", worst["lnq"])
    p_ref = target(case, got["theta"])
    assert same_pattern(got["lnp"], p_ref), (label, "lnp", "-inf pattern", int(np.isneginf(got["lnp"]).sum()), int(np.isneginf(p_ref).sum()))
    fin = np.isfinite(p_ref)
    worst["lnp"] = _ratio(np.abs(got["lnp"][fin] - p_ref[fin]), 1e-9 * np.maximum(1.0, np.abs(p_ref[fin])))
    assert worst["lnp"] <= 1.0, (label, "lnp", worst["lnp"])
    c_ref = float(target(case, centre[None, :])[0])
    assert same_pattern(got["lnp_centre"], c_ref) and (not np.isfinite(c_ref) or abs(got["lnp_centre"] - c_ref) <= 1e-9 * max(1.0, abs(c_ref))), \
        (label, "lnp_centre", got["lnp_centre"], c_ref)
    if got["status"] == 2 or not c_ref > -np.inf:
        assert got["status"] == 2 and not c_ref > -np.inf, (label, "status", got["status"], c_ref)
        for k in ("lnZ", "lnZ_se", "lnZ_psis", "khat", "ess", "mean", "sd", "cov", "lw"):
            assert np.all(np.isnan(got[k])), (label, "status 2", k)
        assert got["n_out"] == 0, (label, "status 2", "n_out")
        return worst
    assert got["n_out"] == int((~fin).sum()), (label, "n_out", got["n_out"], int((~fin).sum()))
    if not fin.any():
        assert np.isneginf(got["lnZ"]), (label, "lnZ", got["lnZ"])
        for k in ("lnZ_se", "lnZ_psis", "khat", "ess", "mean", "sd", "cov", "lw"):
            assert np.all(np.isnan(got[k])), (label, "every draw rejected", k)
        return worst
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(got["lnp"]), got["lnp"] - got["lnq"], -np.inf)
    lw_ref, khat_ref, _ = psis_weights(r)
    assert same_pattern(got["khat"], khat_ref), (label, "khat", got["khat"], khat_ref)
    if np.isfinite(khat_ref):
        worst["khat"] = abs(got["khat"] - khat_ref) / (1e-10 * max(1.0, abs(khat_ref)))
        assert worst["khat"] <= 1.0, (label, "khat", got["khat"], khat_ref, worst["khat"])
    assert same_pattern(got["lw"], lw_ref), (label, "lw", "-inf pattern")
    f = np.isfinite(lw_ref)
    worst["lw"] = _ratio(np.abs(got["lw"][f] - lw_ref[f]), 1e-11 * np.maximum(1.0, np.abs(lw_ref[f])))
    assert worst["lw"] <= 1.0, (label, "lw", worst["lw"])
    o = summaries(r, got["lw"], got["theta"])
    bars = _moment_bars(o, S)
    for k in ("lnZ", "lnZ_psis", "lnZ_se", "ess", "mean", "sd", "cov"):
        g = np.asarray(got[k], dtype=np.float64)
        w = np.asarray(o[k], dtype=LD)
        assert g.shape == w.shape and np.isfinite(g).all(), (label, k, "shape or not finite", g)
        worst[k] = _ratio(np.abs(g - w), bars[k])
        assert worst[k] <= 1.0, (label, k, worst[k])
    assert np.array_equal(got["cov"], got["cov"].T), (label, "cov", "not symmetric")
    return worst


def from_record(rec):
    """a ``vamp_amd.laplace.LaplaceRecord`` made with every per-sample output as the dict ``check`` takes"""
    return {k: getattr(rec, k) for k in ("lnZ", "lnZ_se", "lnZ_psis", "khat", "ess", "lnp_centre", "n_out", "status", "mean", "sd", "cov",
                                         "theta", "z", "lnp", "lnq", "lw")}


# ---- the inputs the tests share ----------------------------------------------------------------------------------
QUAD_LNZ = 8.227          # tests/test_evidence.py: the midpoint rule at 80^3 and 160^3 points
QUAD_SEED = 20110101      # the seed of the quadrature bound, on the CPU and on the device
_cache = {}


def map_and_cov(x, flux, noise, n_comp, mode, start):
    """(MAP, Fisher covariance at it) without a GPU: scipy's fmin on the oracle's log_prob, then fisher_ref"""
    import fisher_ref
    from scipy.optimize import fmin
    R = vo.Region(x=x, flux=flux, noise=noise, n_comp=n_comp, mode=mode)
    best = fmin(lambda t: -vo.log_prob(R, t), np.asarray(start, dtype=np.float64), xtol=1e-6, ftol=1e-9, maxiter=20000, maxfun=20000, disp=False)
    f, J = fisher_ref.jacobian(x, best, n_comp, mode)
    return best, fisher_ref.from_jacobian(J, f, flux, noise, best, n_comp, mode)["cov"]


def quadrature_case(n_samples=4096, inflate=1.5, seed=QUAD_SEED):
    """the one-line quadrature case of tests/test_evidence.py (24 pixels, ln Z = 8.227) with the proposal N(MAP, inflate^2
    Fisher covariance)"""
    key = ("quad", n_samples, inflate, seed)
    if key not in _cache:
        x, flux, noise = evidence_ref.gauss_line_data(24, [(1.2, 11.3, 2.5)], 0.1, 3)
        if "quad_map" not in _cache:
            _cache["quad_map"] = map_and_cov(x, flux, noise, 1, 0, [1.2, 11.3, 2.5])
        best, cov = _cache["quad_map"]
        _cache[key] = make_case(x, flux, noise, 1, 0, best, np.linalg.cholesky(inflate ** 2 * cov), n_samples, seed)
    return _cache[key]


def quadrature_run():
    """the restatement of ``quadrature_case()``, computed once"""
    if "quad_run" not in _cache:
        _cache["quad_run"] = run(quadrature_case())
    return _cache["quad_run"]


def voigt_edge_case(S=400, seed=77):
    """one Voigt line whose L_fwhm sits on its lower bound 0: the proposal is symmetric in L, so about half the draws
    fall outside the prior"""
    x = np.arange(24.0)
    tau = vo.voigt_function(x, 11.3, 1.2, 0.0, 5.0)
    flux = np.exp(-tau) + 0.05 * np.random.default_rng(3).standard_normal(24)
    centre = np.array([1.2, 11.3, 0.0, 5.0])
    chol = np.linalg.cholesky(np.diag([0.05, 0.1, 0.3, 0.2]) ** 2 + 0.001)
    return make_case(x, flux, np.full(24, 0.05), 1, 1, centre, chol, S, seed, region_id=4)


class FakeLibrary:
    """stands in for ``vamp_amd.laplace._call`` in the wiring tests: counts the calls and answers with made-up numbers
    that depend on the group only (no sampling).  ``lnZ_of`` / ``khat_of``: functions of n_comp, for the ladder tests"""

    def __init__(self, lnZ_of=None, khat_of=None):
        self.calls, self.seen = [], []
        self.lnZ_of = lnZ_of or (lambda k: -5.0 * abs(k - 2))
        self.khat_of = khat_of or (lambda k: 0.3)

    def __call__(self, device, xs, fluxes, noises, n_comp, modes, sample_sd, bounds, region_ids, centres, chols, n_samples, seed, want=(), **kw):
        G = len(xs)
        self.calls.append(G)
        self.seen.append({"centres": [np.array(c) for c in centres], "chols": [np.array(c) for c in chols], "region_ids": list(region_ids),
                          "bounds": list(bounds), "n_samples": n_samples, "seed": seed, "noises": list(noises)})
        dims = [(4 if m == 1 else 3) * k + sd for m, k, sd in zip(modes, n_comp, sample_sd)]
        bad = [not np.isfinite(np.tril(c)).all() for c in chols]
        nan_if = lambda v, b: np.nan if b else v
        out = {"lnZ": np.array([nan_if(self.lnZ_of(k), b) for k, b in zip(n_comp, bad)]), "lnZ_se": np.array([nan_if(0.01, b) for b in bad]),
               "lnZ_psis": np.array([nan_if(self.lnZ_of(k) + 0.001, b) for k, b in zip(n_comp, bad)]),
               "khat": np.array([nan_if(self.khat_of(k), b) for k, b in zip(n_comp, bad)]), "ess": np.array([nan_if(0.5 * n_samples, b) for b in bad]),
               "lnp_centre": np.array([nan_if(3.0, b) for b in bad]), "n_out": np.zeros(G, dtype=np.int32), "status": np.array(bad, dtype=np.int32),
               "mean": np.concatenate([np.full(c.size, np.nan) if b else np.asarray(c) + 0.01 for c, b in zip(centres, bad)]),
               "sd": np.concatenate([np.full(d, np.nan) if b else np.sqrt(np.diag(np.tril(c) @ np.tril(c).T)) for c, d, b in zip(chols, dims, bad)]),
               "cov": np.concatenate([(np.full((d, d), np.nan) if b else np.tril(c) @ np.tril(c).T).ravel() for c, d, b in zip(chols, dims, bad)])}
        for k in want:
            out[k] = [np.zeros((n_samples, d)) if k in ("theta", "z") else np.zeros(n_samples) for d in dims]
        return out
