"""Exact references for the STATISTICS of the stretch move (numpy / scipy only), and the checks built on them.

Every other sampler test compares trajectories with the oracle's restatement of the move; the rules of that restatement
(the (D - 1) ln z factor, g(z), the partner from the frozen colour, rejection at the prior's walls, NaN -> -inf) were
written from the published algorithm, so an error shared by both sides is invisible to them.  The tests built on this
module (tests/test_sampler_stats.py, tests/test_gpu_sampler_stats.py) need no restatement of the move at all:

  invariance   W walkers that START as independent draws from the target pi are still independent draws from pi after
               any number of correct steps (DESIGN.md "Sampler statistics"), so sqrt(N) D_N of the N final values of a
               parameter against its exact marginal CDF follows Kolmogorov's law: P(lambda > 3.3) = 2 exp(-2 3.3^2) = 7e-10.
  acceptance   p_acc = E[min(1, z^(D-1) pi(y) / pi(x_m))], x_m, x_p ~ pi, z ~ g, y = x_p + z (x_m - x_p): a plain integral,
               computed here by direct Monte Carlo with no sampler involved.

Two targets have exact draws and exact marginals: the prior itself (a product: A ~ x e^-x, c and the widths uniform),
reached with a flat likelihood, and the posterior of ONE Gaussian line on 24 pixels by quadrature (fixed noise, D = 3,
and the product's default free sd, D = 4).  ``numpy_stretch`` is a move of the library's semantics drawn from numpy's
generator, and the same move with one rule broken at a time: the tests run it to show that every bar below can be met
and that every broken rule misses one.
"""
import functools
import json
import math
import os

import numpy as np
from scipy.interpolate import CubicSpline

from oracle import vamp_oracle as vo
import evidence_ref as ref

# ---- the bars (DESIGN.md "Sampler statistics") ------------------------------------------------------------------------
KS_BAR = 3.3            # sqrt(N) D_N; Kolmogorov tail 2 exp(-2 * 3.3^2) = 7e-10 per comparison
ACC_SIGMAS = 5.0        # |acc - p_acc| <= 5 sqrt(se_run^2 + se_ref^2)
SE_RUN_CAP = 3e-4       # conditions, not measurements: a leg whose own scatter is larger proves nothing
SE_REF_CAP = 2e-4
CORR_BAR = 6.0          # |corr| sqrt(N) of two independent parameters is N(0, 1): P(> 6) = 2e-9 per pair
EPS_FRACTION = 0.1      # the quadrature's CDF error may use a tenth of the KS bar: eps <= 0.1 * 3.3 / sqrt(N)
BROKEN = ("dm2", "zunif", "leak", "stale")


def ks_lambda(samples, cdf):
    """sqrt(N) D_N: the two-sided Kolmogorov-Smirnov statistic of ``samples`` against the CDF ``cdf``, scaled"""
    s = np.sort(np.asarray(samples, dtype=np.float64).ravel())
    n = s.size
    u = np.asarray(cdf(s), dtype=np.float64)
    i = np.arange(1, n + 1, dtype=np.float64)
    return math.sqrt(n) * max(float(np.max(i / n - u)), float(np.max(u - (i - 1.0) / n)))


def _stretch_z(u, a):
    t = (a - 1.0) * u + 1.0
    return t * t / a


def acceptance_reference(draw, logp, D, n, a=2.0, rng=None, chunk=1 << 18):
    """(p_acc, standard error) of one stretch proposal at stationarity by direct Monte Carlo over n proposals:
    x_m, x_p = draw(k, rng) independent exact draws, z ~ g, y = x_p + z (x_m - x_p), min(1, z^(D-1) pi(y) / pi(x_m))"""
    rng = np.random.default_rng(0) if rng is None else rng
    s1 = s2 = 0.0
    done = 0
    while done < n:
        k = min(chunk, n - done)
        xm, xp = draw(k, rng), draw(k, rng)
        z = _stretch_z(rng.random(k), a)
        y = xp + z[:, None] * (xm - xp)
        with np.errstate(all="ignore"):
            p = np.exp(np.minimum(0.0, (D - 1.0) * np.log(z) + logp(y) - logp(xm)))
        p = np.where(np.isnan(p), 0.0, p)
        s1 += float(p.sum())
        s2 += float((p * p).sum())
        done += k
    mean = s1 / n
    return mean, math.sqrt(max(s2 / n - mean * mean, 0.0) / n)


def acceptance_reference_to(draw, logp, D, se=0.95 * SE_REF_CAP, a=2.0, seed=0):
    """acceptance_reference with the number of proposals chosen from a pilot of 2^18 so that its error is ``se``"""
    rng = np.random.default_rng(seed)
    _, se0 = acceptance_reference(draw, logp, D, 1 << 18, a, rng)
    n = int(math.ceil((1 << 18) * (1.05 * se0 / se) ** 2)) + 1024
    return acceptance_reference(draw, logp, D, n, a, rng)


# ---- target 1: the prior of a region (oracle.vamp_oracle.log_prior) ------------------------------------------------------
class RegionPrior:
    """The prior of K lines on the abscissa x, per oracle.vamp_oracle.log_prior: A ~ x e^-x (Gamma(2, 1), CDF
    1 - (1 + x) e^-x), c ~ U(x[0], x[-1]), sigma ~ U(0, sigma_max) or L, G ~ U(0, fwhm_max), sd ~ U(0, 1)."""

    def __init__(self, mode, K, x, sample_sd=False):
        lo, hi = float(x[0]), float(x[-1])
        smax = (hi - lo) / 2.0
        widths = [(0.0, smax)] if mode == vo.MODE_GAUSS3 else [(0.0, smax * vo.FWHM_PER_SIGMA)] * 2
        self.dims = ([None, (lo, hi)] + widths) * K + ([(0.0, 1.0)] if sample_sd else [])      # None: the x e^-x prior
        self.D = len(self.dims)
        self.eps = 0.0
        self._amp = np.array([d is None for d in self.dims])
        self._lo = np.array([0.0 if d is None else d[0] for d in self.dims])
        self._hi = np.array([np.inf if d is None else d[1] for d in self.dims])
        self._const = -float(sum(math.log(d[1] - d[0]) for d in self.dims if d is not None))

    def draw(self, n, rng):
        X = np.empty((n, self.D))
        for d, spec in enumerate(self.dims):
            X[:, d] = rng.gamma(2.0, 1.0, n) if spec is None else rng.uniform(spec[0], spec[1], n)
        return X

    def cdf(self, d):
        spec = self.dims[d]
        if spec is None:
            return lambda v: np.where(v > 0, 1.0 - (1.0 + np.maximum(v, 0.0)) * np.exp(-np.maximum(v, 0.0)), 0.0)
        return lambda v: np.clip((v - spec[0]) / (spec[1] - spec[0]), 0.0, 1.0)

    def logp(self, X):
        """ln prior of X[n, D]; -inf outside the closed boxes and for A <= 0"""
        X = np.asarray(X, dtype=np.float64)
        with np.errstate(all="ignore"):
            A = X[:, self._amp]
            out = self._const + np.sum(np.log(A) - A, axis=1)
            ok = np.all((X >= self._lo) & (X <= self._hi), axis=1)
        return np.where(ok & np.isfinite(out), out, -np.inf)


# ---- target 2: the posterior of one Gaussian line by quadrature ------------------------------------------------------------
LINE_DATA = (24, [(1.2, 11.3, 2.5)], 0.1, 3)      # evidence_ref.gauss_line_data's arguments (tests/test_gpu_evidence.py)
# The box holds all but this much of the posterior's mass.  Fixed noise: 1e-9.  Free sd: the marginal of (A, c, sigma) falls
# like S^-(P-1)/2, not exponentially, and ~1e-5 of the mass is spread over the WHOLE prior box (a model without a line,
# sd ~ 0.3): no box smaller than the prior holds all but 1e-9.  There the cut is 1e-4, and the cut mass is added to eps: a
# CDF of the cut density differs from the exact one by at most the mass cut.
MASS_CUT = {False: 1e-9, True: 1e-4}
A_MAX = 12.0                                      # first box of the amplitude, as evidence_ref.quadrature_lnZ


class GaussLinePosterior:
    """Posterior of (A, c, sigma[, sd]) for the data of LINE_DATA under the oracle's prior and likelihood: fixed noise
    (D = 3: -chi^2 / 2) or ``sample_sd`` (D = 4: noise = 1 as VPfit uploads it, P/2 ln(t / 2 pi) - t S / 2, t = 1 / sd^2,
    sd ~ U(0, 1)).  The midpoint rule on a box cut to all but 1e-9 of the mass; the integrand vanishes at the box's faces,
    so the rule converges geometrically in the other axes and a marginal's density at the nodes is a point value: its CDF
    is the antiderivative of the cubic spline through them.  ``eps`` = sup |CDF at n nodes - CDF at 2 n nodes| over the
    parameters, plus the mass the box cuts; n is doubled until eps <= 0.1 * 3.3 / sqrt(N) for the N samples the caller will
    test; the 2 n grid serves."""

    def __init__(self, sample_sd, N, n0=32):
        self.sample_sd = bool(sample_sd)
        self.x, self.flux, self.noise_fixed = ref.gauss_line_data(*LINE_DATA)
        self.noise = np.ones_like(self.x) if self.sample_sd else self.noise_fixed
        self.P = self.x.size
        self.D = 4 if self.sample_sd else 3
        self.c_lo, self.c_hi = float(self.x[0]), float(self.x[-1])
        self.s_max = (self.c_hi - self.c_lo) / 2.0
        self.eps_bar = EPS_FRACTION * KS_BAR / math.sqrt(N)
        self.box = self._find_box()
        n = n0
        coarse = self._grid(self.box, n)
        while True:
            fine = self._grid(self.box, 2 * n)
            probe = [np.linspace(lo, hi, 4001) for lo, hi in self.box]
            self.eps_quad = max(float(np.max(np.abs(coarse["cdf"][d](probe[d]) - fine["cdf"][d](probe[d])))) for d in range(self.D))
            self.eps = self.eps_quad + MASS_CUT[self.sample_sd]
            if self.eps <= self.eps_bar or 2 * n >= 256:
                break
            n, coarse = 2 * n, fine
        self.n = 2 * n
        self._g = fine
        self._proposed, self._excess = 0, 0.0
        self.lnZ = fine["lnZ"]

    # the integrand ---------------------------------------------------------------------------------------------------
    def _sumsq(self, A, c, s):
        """S[A, c, s] = sum over pixels of (flux - exp(-A exp(-((x - c) / s)^2 / 2)))^2 on the product grid"""
        prof = np.exp(-0.5 * ((self.x[None, None, :] - c[:, None, None]) / s[None, :, None]) ** 2)          # [c, s, P]
        S = np.empty((A.size, c.size, s.size))
        for i, amp in enumerate(A):
            S[i] = np.sum((self.flux - np.exp(-amp * prof)) ** 2, axis=2)
        return S

    def logp(self, X):
        """ln posterior (unnormalised, the library's lnprob without include_norm) of X[n, D]; -inf outside the prior"""
        X = np.asarray(X, dtype=np.float64)
        with np.errstate(all="ignore"):
            A, c, s = X[:, 0], X[:, 1], X[:, 2]
            m = np.exp(-A[:, None] * np.exp(-0.5 * ((self.x[None, :] - c[:, None]) / s[:, None]) ** 2))
            S = np.sum((self.flux[None, :] - m) ** 2, axis=1)
            lp = np.log(A) - A - math.log(self.c_hi - self.c_lo) - math.log(self.s_max)
            ok = (A > 0) & (c >= self.c_lo) & (c <= self.c_hi) & (s >= 0) & (s <= self.s_max)
            if self.sample_sd:
                sd = X[:, 3]
                ok &= (sd > 0) & (sd <= 1.0)
                out = lp + self.P * 0.5 * np.log(1.0 / (sd * sd) / (2.0 * math.pi)) - 0.5 * S / (sd * sd)
            else:
                out = lp - 0.5 * S / self.noise_fixed[0] ** 2
        return np.where(ok & np.isfinite(out), out, -np.inf)

    # the quadrature --------------------------------------------------------------------------------------------------
    def _grid(self, box, n):
        """midpoint rule at n nodes per axis on ``box``: cell masses, marginal CDFs, ln Z"""
        h = [(hi - lo) / n for lo, hi in box]
        node = [lo + (np.arange(n) + 0.5) * hd for (lo, _), hd in zip(box, h)]
        A, c, s = node[:3]
        S = self._sumsq(A, c, s)
        lpa = (np.log(A) - A)[:, None, None]
        const = -math.log(self.c_hi - self.c_lo) - math.log(self.s_max)
        if self.sample_sd:
            sd = node[3]
            top = float(np.max(lpa)) + float(np.max(-self.P * np.log(sd) - 0.5 * S.min() / sd ** 2))      # >= the maximum: no overflow
            w3 = np.zeros_like(S)
            msd = np.empty(n)
            for l, v in enumerate(sd):
                w = np.exp(lpa - self.P * math.log(v) - 0.5 * S / (v * v) - top)
                msd[l] = w.sum()
                w3 += w
            const += -0.5 * self.P * math.log(2.0 * math.pi)
        else:
            expo = lpa - 0.5 * S / self.noise_fixed[0] ** 2
            top = float(expo.max())
            w3 = np.exp(expo - top)
            const += -0.5 * float(np.sum(np.log(2.0 * math.pi * self.noise_fixed ** 2)))      # include_norm, as quadrature_lnZ
        total = float(w3.sum())
        marg = [w3.sum(axis=(1, 2)), w3.sum(axis=(0, 2)), w3.sum(axis=(0, 1))] + ([msd] if self.sample_sd else [])
        cdf = [self._spline_cdf(box[d], node[d], marg[d] / (total * h[d])) for d in range(self.D)]
        return {"n": n, "h": h, "node": node, "w3": w3, "S": S, "marg": [m / total for m in marg], "cdf": cdf,
                "lnZ": top + math.log(total) + sum(math.log(v) for v in h) + const}

    @staticmethod
    def _spline_cdf(bounds, node, pdf):
        """CDF from the density's values at the nodes: antiderivative of their cubic spline (density 0 at the box's faces),
        0 below the box, 1 above, normalised to 1 at the upper face"""
        lo, hi = bounds
        F = CubicSpline(np.r_[lo, node, hi], np.r_[0.0, pdf, 0.0]).antiderivative()
        top = float(F(hi))
        return lambda v: np.clip(F(np.clip(v, lo, hi)) / top, 0.0, 1.0)

    def _find_box(self):
        """shrink the prior's box (A up to A_MAX) onto the posterior: per axis, drop the cells whose cumulated marginal
        mass from either end is below MASS_CUT / (2 D), keep two cells of margin, repeat until the box stops shrinking"""
        box = [(0.0, A_MAX), (self.c_lo, self.c_hi), (0.0, self.s_max)] + ([(0.0, 1.0)] if self.sample_sd else [])
        first = list(box)
        tail = MASS_CUT[self.sample_sd] / (2 * self.D)
        for _ in range(12):
            n = 64
            g = self._grid(box, n)
            new = []
            for d in range(self.D):
                cum = np.cumsum(g["marg"][d])
                i0 = int(np.searchsorted(cum, tail))                       # first cell that brings the mass above the cut
                i1 = int(np.searchsorted(cum, 1.0 - tail))
                lo = max(box[d][0] + (i0 - 2) * g["h"][d], first[d][0])
                hi = min(box[d][0] + (i1 + 3) * g["h"][d], first[d][1])
                new.append((lo, hi))
            vol = np.prod([(b[1] - b[0]) / (a[1] - a[0]) for a, b in zip(new, box)])
            box = new
            if vol > 0.7:
                break
        return box

    # exact draws -----------------------------------------------------------------------------------------------------
    ENVELOPE = 8.0

    def _propose(self, n, rng):
        """a cell of the grid chosen by its mass, plus uniform jitter within the cell: (points, their cells' midpoints).
        The proposal's density is constant on a cell and proportional to the posterior at its midpoint."""
        g = self._g
        if "cum" not in g:
            g["cum"] = np.cumsum(g["w3"].ravel())
        cum = g["cum"]
        cell = np.minimum(np.searchsorted(cum, rng.random(n) * cum[-1], side="right"), cum.size - 1)
        idx = np.unravel_index(cell, g["w3"].shape)
        X, mid = np.empty((n, self.D)), np.empty((n, self.D))
        for d in range(3):
            mid[:, d] = g["node"][d][idx[d]]
        if self.sample_sd:
            sd = g["node"][3]
            S = g["S"].ravel()[cell]
            for b in range(0, n, 1 << 14):                                # sd given the cell: its conditional on the sd nodes
                e = min(n, b + (1 << 14))
                lw = -self.P * np.log(sd)[None, :] - 0.5 * S[b:e, None] / sd[None, :] ** 2
                cw = np.cumsum(np.exp(lw - lw.max(axis=1, keepdims=True)), axis=1)
                k = np.minimum((cw < (rng.random(e - b) * cw[:, -1])[:, None]).sum(axis=1), sd.size - 1)
                mid[b:e, 3] = sd[k]
        for d in range(self.D):
            X[:, d] = mid[:, d] + (rng.random(n) - 0.5) * g["h"][d]
        return X, mid

    def draw(self, n, rng):
        """n exact draws: proposals of _propose, accepted with probability pi(x) / (ENVELOPE pi(midpoint of x's cell)).
        Exact wherever pi varies by less than ENVELOPE inside a cell; ``draw_excess`` is the share of the posterior's mass
        the envelope has cut so far (far tails: the self-test holds it below 1e-6)."""
        out, got = [], 0
        while got < n:
            k = int((n - got) * self.ENVELOPE * 1.1) + 1024
            X, mid = self._propose(k, rng)
            with np.errstate(all="ignore"):
                lr = self.logp(X) - self.logp(mid)
            self._proposed += k
            self._excess += float(np.sum(np.maximum(np.exp(lr) - self.ENVELOPE, 0.0)))
            keep = np.log(rng.random(k)) < lr - math.log(self.ENVELOPE)
            out.append(X[keep])
            got += int(keep.sum())
        return np.concatenate(out)[:n]

    @property
    def draw_excess(self):
        return self._excess / max(self._proposed, 1)

    def cdf(self, d):
        return self._g["cdf"][d]


@functools.lru_cache(maxsize=None)
def gauss_line_posterior(sample_sd, N):
    return GaussLinePosterior(sample_sd, N)


# ---- a numpy stretch move of the library's semantics, and the same move with one rule broken ------------------------------
def numpy_stretch(logp, X0, R, W, T, rng, a=2.0, broken=None):
    """T steps of R independent ensembles of W walkers (X0[R * W, D], ensemble-major) under the library's rules: the
    ensemble is split into two colours by a permutation that does not look at the state, each colour moves in turn, every
    mover draws its partner uniformly from the frozen colour, z = ((a - 1) u + 1)^2 / a, accept iff
    ln u' < (D - 1) ln z + ln pi(y) - ln pi(x); ln pi = NaN counts as -inf.  ``broken``: "dm2" exponent D - 2; "zunif"
    z uniform on [1 / a, a]; "leak" a proposal outside the support is accepted with the walker's last finite ln pi;
    "stale" ln pi is not updated on accept.  Returns (X, lnp, n_accept[R * W])."""
    assert broken in (None,) + BROKEN and W % 2 == 0
    X = np.array(X0, dtype=np.float64)
    N, D = X.shape
    assert N == R * W
    lnp = np.asarray(logp(X), dtype=np.float64).copy()
    nacc = np.zeros(N, dtype=np.int64)
    base = (np.arange(R) * W)[:, None]
    h = W // 2
    expo = D - 2.0 if broken == "dm2" else D - 1.0
    for _ in range(T):
        perm = rng.permuted(np.tile(np.arange(W), (R, 1)), axis=1) + base
        for act2, comp2 in ((perm[:, :h], perm[:, h:]), (perm[:, h:], perm[:, :h])):
            act = act2.ravel()
            partner = np.take_along_axis(comp2, rng.integers(0, h, (R, h)), axis=1).ravel()
            u = rng.random(act.size)
            z = 1.0 / a + (a - 1.0 / a) * u if broken == "zunif" else _stretch_z(u, a)
            Xc = X[partner]
            q = Xc - (Xc - X[act]) * z[:, None]
            lq = np.asarray(logp(q), dtype=np.float64)
            lq = np.where(np.isnan(lq), -np.inf, lq)
            cur = lnp[act]
            if broken == "leak":
                lq = np.where(np.isfinite(lq), lq, cur)
            with np.errstate(all="ignore"):
                diff = expo * np.log(z) + lq - cur
                acc = np.log(rng.random(act.size)) < diff
            acc &= ~np.isnan(diff)
            X[act[acc]] = q[acc]
            if broken != "stale":
                lnp[act[acc]] = lq[acc]
            nacc[act[acc]] += 1
    return X, lnp, nacc


# ---- the figures of one leg and its bars -------------------------------------------------------------------------------
def leg_figures(X, nacc, R, W, T, target, p_ref, se_ref, corr):
    """X[R * W, D] final positions (ensemble-major), nacc[R * W] accepted moves of T steps.  Returns the figures the
    bars are set on: lambda per parameter, the acceptance, se_run = scatter of the R ensembles' mean acceptances / sqrt(R),
    the distance to the reference in units of the joint error, the largest |corr| sqrt(N)."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    lam = np.array([ks_lambda(X[:, d], target.cdf(d)) for d in range(D)])
    per = np.asarray(nacc, dtype=np.float64).reshape(R, W).mean(axis=1) / T
    acc, se_run = float(per.mean()), float(per.std(ddof=1) / math.sqrt(R))
    fig = {"N": N, "D": D, "lambda": lam, "ks_bar": KS_BAR + math.sqrt(N) * target.eps, "acc": acc, "se_run": se_run,
           "p_ref": p_ref, "se_ref": se_ref, "acc_dev": abs(acc - p_ref) / math.sqrt(se_run ** 2 + se_ref ** 2), "corr": None}
    if corr:
        cm = np.corrcoef(X, rowvar=False)
        fig["corr"] = float(np.max(np.abs(cm[~np.eye(D, dtype=bool)]))) * math.sqrt(N)
    return fig


def format_figures(label, fig):
    lam = fig["lambda"]
    s = "%-44s N %6d D %2d  max lambda %5.2f (bar %.2f)  acc %.5f +- %.5f  ref %.5f +- %.5f  dev %5.2f se" % (
        label, fig["N"], fig["D"], lam.max(), fig["ks_bar"], fig["acc"], fig["se_run"], fig["p_ref"], fig["se_ref"], fig["acc_dev"])
    if fig["corr"] is not None:
        s += "  max |corr| sqrt(N) %.2f" % fig["corr"]
    if fig["D"] > 16:
        s += "  [KS has little power at this D: acceptance carries the leg]"
    return s


def failed_bars(fig):
    """the bars a leg's figures miss: a subset of {"ks", "acc", "corr"}; the two conditions are asserted apart"""
    out = set()
    if not fig["lambda"].max() < fig["ks_bar"]:
        out.add("ks")
    if not fig["acc_dev"] <= ACC_SIGMAS:
        out.add("acc")
    if fig["corr"] is not None and not fig["corr"] < CORR_BAR:
        out.add("corr")
    return out


def assert_leg(label, fig):
    """print the figures, then assert the conditions and the bars"""
    print(format_figures(label, fig))
    assert fig["se_run"] <= SE_RUN_CAP and fig["se_ref"] <= SE_REF_CAP, (label, "conditions", fig["se_run"], fig["se_ref"])
    assert fig["lambda"].max() < fig["ks_bar"], (label, "KS", fig["lambda"])
    assert fig["acc_dev"] <= ACC_SIGMAS, (label, "acceptance", fig["acc"], fig["p_ref"], fig["acc_dev"])
    if fig["corr"] is not None:
        assert fig["corr"] < CORR_BAR, (label, "correlation", fig["corr"])


# ---- the legs: targets, references, and a run through a context (libvamp_hip.so or the host ABI) -------------------------
PRIOR_LEGS = {       # name: (mode, K, P, T)
    "a": (vo.MODE_GAUSS3, 1, 8, 200), "b": (vo.MODE_VOIGT4, 1, 8, 200), "c": (vo.MODE_VOIGT4, 4, 40, 800),
    "d": (vo.MODE_VOIGT4, 3, 128, 800), "e12": (vo.MODE_GAUSS3, 12, 40, 800), "e17": (vo.MODE_VOIGT4, 17, 40, 800),
    "f": (vo.MODE_VOIGT4, 2, 600, 200),
}
POSTERIOR_T = 100


GOLDEN_ACCEPTANCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_stats_acceptance.json")


def _leg_targets():
    """every leg's (name, target, seed of its acceptance integral)"""
    out = []
    for name, (mode, K, P, _) in PRIOR_LEGS.items():
        out.append((name, RegionPrior(mode, K, np.arange(float(P))), 1000 + P + K))
    return out + [("post-fixed", gauss_line_posterior(False, 65536), 2000), ("post-sd", gauss_line_posterior(True, 65536), 2001)]


def write_golden():
    """the acceptance integral of every leg to se <= 0.95 * SE_REF_CAP, as [p_acc, se] (minutes; `python tests/sampler_stats.py`).
    tests/test_sampler_stats.py holds the committed values against a fresh integral with another seed."""
    rec = {}
    for name, target, seed in _leg_targets():
        rec[name] = list(acceptance_reference_to(target.draw, target.logp, target.D, seed=seed))
        print(name, rec[name])
    with open(GOLDEN_ACCEPTANCE, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


@functools.lru_cache(maxsize=None)
def _golden_acceptance():
    with open(GOLDEN_ACCEPTANCE) as f:
        return {k: (float(v[0]), float(v[1])) for k, v in json.load(f).items()}


@functools.lru_cache(maxsize=None)
def prior_leg(name):
    """(data, target, (p_acc, se)) of a prior leg: flat likelihood (flux = 1, noise = 1e8: |d ln L| <= P * 5e-17), x = 0 .. P - 1"""
    mode, K, P, T = PRIOR_LEGS[name]
    x = np.arange(float(P))
    target = RegionPrior(mode, K, x)
    data = dict(x=x, flux=np.ones(P), noise=np.full(P, 1e8), K=K, mode=mode, sample_sd=False, T=T)
    return data, target, _golden_acceptance()[name]


@functools.lru_cache(maxsize=None)
def posterior_leg(sample_sd, N):
    """(data, target, (p_acc, se)) of the one-Gaussian-line posterior, fixed noise or free sd, with the quadrature's eps
    sized for N samples"""
    target = gauss_line_posterior(bool(sample_sd), N)
    data = dict(x=target.x, flux=target.flux, noise=target.noise, K=1, mode=vo.MODE_GAUSS3, sample_sd=bool(sample_sd), T=POSTERIOR_T)
    return data, target, _golden_acceptance()["post-sd" if sample_sd else "post-fixed"]


def run_context(ctx, data, X0, R, W, seed, resident, T=None):
    """R copies of the leg's region in ``ctx`` (their draws are keyed by the region index: independent replicas), walkers
    started at X0[R * W, D], T steps.  Returns (X[R * W, D], lnprob, n_accept, timed intervals, classes of region 0)."""
    T = data["T"] if T is None else T
    ctx.set_option("resident", resident)
    try:
        ctx.set_regions([data["x"]] * R, [data["flux"]] * R, [data["noise"]] * R, data["K"], mode=data["mode"], sample_sd=data["sample_sd"])
        kinds, _ = ctx.region_classes()
        assert len(set(kinds)) == 1
        D = X0.shape[1]
        ctx.sampler_init([np.ascontiguousarray(X0[r * W:(r + 1) * W]) for r in range(R)], seed=seed)
        ctx.kernel_timing(True)
        ctx.run(T, store_chain=False)
        _, intervals = ctx.kernel_timing(False)
        X, lnp, nacc, step = ctx.get_state()
    finally:
        ctx.set_option("resident", 1)
    assert step == T
    if R > 1:
        X, lnp, nacc = np.concatenate(X), np.concatenate(lnp), np.concatenate(nacc)
    return X.reshape(R * W, D), lnp, nacc, intervals, kinds[0]


def assert_state_consistent(ctx, X, lnp, R, W, rel):
    """the returned lnprob is ctx's lnprob of the returned positions (|d| <= rel max(1, |lnprob|)); no walker at -inf"""
    assert np.all(np.isfinite(lnp)), "a walker sits at -inf or NaN"
    again = ctx.lnprob_all([X[r * W:(r + 1) * W] for r in range(R)]).ravel() if R > 1 else ctx.lnprob(X)
    err = float(np.max(np.abs(again - lnp) / np.maximum(1.0, np.abs(lnp))))
    print("    state: max |lnprob(returned X) - returned lnprob| / max(1, |lnprob|) = %.3g (bar %.1g)" % (err, rel))
    assert err <= rel, err


if __name__ == "__main__":
    write_golden()
