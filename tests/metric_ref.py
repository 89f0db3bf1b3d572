"""numpy restatement of include/vamp_metric.h: the scaling, the cyclic two-sided Jacobi iteration with
its round-robin schedule, sorting, clamps, cov / prec / logdet and the Cholesky factor, in fp64 and in the header's order;
``check`` holds a result -- the library's, or this file's own -- to the restatement evaluated on the result's OWN outputs
of the stage before; the planted errors that ``check`` must catch; the test families; the measured bars.

The library fuses multiply-adds where numpy rounds twice, so nothing here is compared bit for bit with the library but
the counts; every stage has a bar:

    eig                 against the 40-digit eigenvalues of the fixture            measured (``measured_bars``)
    resid, orth         max |B V - V diag(eig)|, max |V^T V - I| of the result     measured
    cov, prec, logdet   the restatement on the result's eig and vec                (D + 2) eps x the sum of the absolute terms
    chol                C C^T against the result's cov                             (D + 1) eps sqrt(cov_aa cov_bb)
    n_low, n_high       the restatement on the result's eig                        exact

A measured bar is MEASURED_FACTOR times the worst error this fp64 restatement itself shows, against the fixture's
eigenvalues or (resid, orth) evaluated in long double, over the cases of the same D -- the error grows with the number
of rotations, so cases of one D are pooled and cases of different D are not -- and at least MIN_BAR_EPS eps ||B||_F
(eps for orth).  It is never taken from the library.
"""
import math
import os

import numpy as np

EPS = 2.0 ** -52
MEASURED_FACTOR = 4.0
MIN_BAR_EPS = 8.0
MAX_DIM, MAX_SWEEPS = 65, 32
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric", "metric_cases.npz")

# planted error -> the stage of ``check`` that must catch it
PLANTS = {"rows rotated but not columns": "resid", "the sign of s flipped in V": "resid", "kind 1 clamps e instead of 1 / e": "counts",
          "the scale left out of cov": "cov", "unsorted vec": "resid"}


def make_case(mat, scale, kind=0, lam_lo=1.0, lam_hi=2.0 ** 40, eig_ref=None, name=""):
    mat = np.array(mat, dtype=np.float64)
    return dict(mat=mat, scale=np.array(scale, dtype=np.float64), kind=int(kind), lam_lo=float(lam_lo), lam_hi=float(lam_hi),
                eig_ref=None if eig_ref is None else np.array(eig_ref, dtype=np.float64), name=name)


def scaled(case):
    """B of the header from the lower triangle of ``mat``"""
    s = case["scale"]
    low = np.tril(case["mat"])
    with np.errstate(all="ignore"):
        b = (s[:, None] * low) * s[None, :] if case["kind"] == 0 else low / (s[:, None] * s[None, :])
    return np.tril(b) + np.tril(b, -1).T


def frobenius(B):
    """||B||_F in the header's order (a product and a sum where the library fuses them)"""
    r = np.zeros(len(B))
    for j in range(B.shape[1]):
        r = r + B[:, j] * B[:, j]
    tot = 0.0
    for v in r:
        tot += float(v)
    return math.sqrt(tot)


def schedule(n, r):
    """(p, q) of the n / 2 disjoint pairs of round r, p < q"""
    idx = np.array([0] + [1 + (r + k - 1) % (n - 1) for k in range(1, n)])
    a, b = idx[:n // 2], idx[::-1][:n // 2]
    return np.minimum(a, b), np.maximum(a, b)


def jacobi(B, n_sweeps, plant=None):
    """(the diagonal [D], V [D, D], sweeps_used, off, tol) of the header's iteration on B"""
    D = len(B)
    n = D + (D & 1)
    A = np.zeros((n, n))
    A[:D, :D] = B
    V = np.eye(n)
    tol = EPS * frobenius(B)
    used = 0
    for _ in range(int(n_sweeps)):
        rotated = False
        for r in range(n - 1):
            p, q = schedule(n, r)
            apq = A[q, p]
            m = np.abs(apq) > tol
            if not m.any():
                continue
            p, q, apq = p[m], q[m], apq[m]
            tau = (A[q, q] - A[p, p]) / (2.0 * apq)
            t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(tau * tau + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            rotated = True
            x, y = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
            if plant != "rows rotated but not columns":
                x, y = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * x - s * y, s * x + c * y
            sv = -s if plant == "the sign of s flipped in V" else s
            x, y = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * x - sv * y, sv * x + c * y
            A[p, q] = 0.0
            A[q, p] = 0.0
        used += 1
        if not rotated:
            break
    off = float(np.max(np.abs(A - np.diag(np.diag(A)))))
    return np.diag(A)[:D].copy(), V[:D, :D].copy(), used, off, tol


def lam_of(eig, kind, plant=None):
    if kind == 0 or plant == "kind 1 clamps e instead of 1 / e":
        return np.array(eig, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(eig > 0.0, 1.0 / np.where(eig > 0.0, eig, 1.0), np.inf)


def clamp(eig, case, plant=None):
    """(lam~, n_low, n_high) from sorted eigenvalues"""
    lam = lam_of(eig, case["kind"], plant)
    return np.minimum(np.maximum(lam, case["lam_lo"]), case["lam_hi"]), int(np.sum(lam < case["lam_lo"])), int(np.sum(lam > case["lam_hi"]))


def _fma(a, b, c):
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(np.float64)


def matrices(eig, vec, case, plant=None):
    """cov, prec, logdet of the header from sorted eig and vec, and the sums of the absolute terms behind each:
    (cov, prec, logdet, cov_terms, prec_terms, logdet_terms)"""
    s = case["scale"]
    D = len(s)
    lt = clamp(eig, case, plant)[0]
    with np.errstate(all="ignore"):
        iw = 1.0 / lt
        cc, pp, ca, pa = (np.zeros((D, D)) for _ in range(4))
        for i in range(D):
            tc, tp = np.outer(vec[:, i] * iw[i], np.ones(D)), np.outer(vec[:, i] * lt[i], np.ones(D))
            vb = np.outer(np.ones(D), vec[:, i])
            cc, pp = _fma(tc, vb, cc), _fma(tp, vb, pp)
            ca, pa = ca + np.abs(tc * vb), pa + np.abs(tp * vb)
        ss = np.ones(D) if plant == "the scale left out of cov" else s
        cov = (ss[:, None] * cc) * ss[None, :]
        prec = (pp / s[:, None]) / s[None, :]
        sl = 0.0
        for v in lt:
            sl += math.log(v)
        sd = 0.0
        for v in s:
            sd += math.log(v)
    low = lambda m: np.tril(m) + np.tril(m, -1).T
    return (low(cov), low(prec), sl - 2.0 * sd, low(np.outer(s, s) * ca), low(pa / np.outer(s, s)),
            float(np.sum(np.abs(np.log(lt))) + 2.0 * np.sum(np.abs(np.log(s)))))


def cholesky(cov):
    """chol of the header (include/vamp_fisher.h's pivot rule on the scaled matrix), or None"""
    D = len(cov)
    dg = np.diag(cov)
    if not np.all((dg > 0) & np.isfinite(dg)):
        return None
    sq = np.sqrt(dg)
    a = np.tril(cov / (sq[:, None] * sq[None, :]))
    thr = D * EPS
    for k in range(D):
        if not a[k, k] > thr:
            return None
        l = math.sqrt(a[k, k])
        a[k, k] = l
        a[k + 1:, k] *= 1.0 / l
        for j in range(k + 1, D):
            a[j:, j] -= a[j:, k] * a[j, k]
    return sq[:, None] * a


def nan_result(D, status):
    nan = np.full((D, D), np.nan)
    return dict(eig=np.full(D, np.nan), vec=nan.copy(), cov=nan.copy(), prec=nan.copy(), chol=nan.copy(), logdet=np.nan, n_low=0, n_high=0,
                sweeps_used=0, off=np.nan, status=status)


def run(case, n_sweeps, plant=None):
    """every output of the header for one matrix"""
    D = len(case["scale"])
    B = scaled(case)
    if not (np.isfinite(np.tril(case["mat"])).all() and np.isfinite(B).all() and np.isfinite(frobenius(B))):
        return nan_result(D, 2)
    dg, V, used, off, tol = jacobi(B, n_sweeps, plant)
    order = np.argsort(dg, kind="stable")
    eig = dg[order]
    vec = V if plant == "unsorted vec" else V[:, order]
    _, n_low, n_high = clamp(eig, case, plant)
    out = nan_result(D, 3)
    out.update(eig=eig, vec=vec, n_low=n_low, n_high=n_high, sweeps_used=used, off=off)
    if off > tol:
        return out
    cov, prec, logdet = matrices(eig, vec, case, plant)[:3]
    chol = cholesky(cov)
    out.update(cov=cov, prec=prec, logdet=logdet, status=0 if chol is not None else 1)
    if chol is not None:
        out["chol"] = chol
    return out


# ---- the bars and the check -------------------------------------------------------------------------------------------
def eigen_errors(res, case):
    """{"eig": against the fixture (None without one), "resid", "orth"} of a result's eig and vec, evaluated in long double"""
    B = scaled(case).astype(LD)
    V, e = res["vec"].astype(LD), res["eig"].astype(LD)
    D = len(e)
    out = {"resid": float(np.max(np.abs(B @ V - V * e[None, :]))), "orth": float(np.max(np.abs(V.T @ V - np.eye(D, dtype=LD)))), "eig": None}
    if case.get("eig_ref") is not None:
        out["eig"] = float(np.max(np.abs(res["eig"] - case["eig_ref"])))
    return out


def measured_bars(cases, n_sweeps=MAX_SWEEPS):
    """{D: {"eig", "resid": relative to ||B||_F, "orth": absolute, "worst": the restatement's own worst figures}} over the
    cases, pooled by D (a case without reference eigenvalues adds to resid and orth only)"""
    worst = {}
    for c in cases:
        res = run(c, n_sweeps)
        assert res["status"] in (0, 1), (c["name"], res["status"])
        e = eigen_errors(res, c)
        nb = frobenius(scaled(c))
        w = worst.setdefault(len(c["scale"]), {"eig": 0.0, "resid": 0.0, "orth": 0.0})
        if nb > 0:
            w["eig"], w["resid"] = max(w["eig"], (e["eig"] or 0.0) / nb), max(w["resid"], e["resid"] / nb)
        w["orth"] = max(w["orth"], e["orth"])
    return {D: {"eig": max(MEASURED_FACTOR * w["eig"], MIN_BAR_EPS * EPS), "resid": max(MEASURED_FACTOR * w["resid"], MIN_BAR_EPS * EPS),
                "orth": max(MEASURED_FACTOR * w["orth"], MIN_BAR_EPS * EPS), "worst": w} for D, w in worst.items()}


def _ratio(err, bar):
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    with np.errstate(all="ignore"):
        return float(np.max(np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf)), initial=0.0))


class StageError(AssertionError):
    def __init__(self, stage, msg):
        super().__init__(f"{stage}: {msg}")
        self.stage = stage


def check(res, case, bars, n_sweeps=MAX_SWEEPS, label=""):
    """Holds one matrix's result (a dict of the header's outputs) to the restatement on its own outputs; ``bars``: the
    entry of ``measured_bars`` for the case's D.  Returns the worst error over its bar per stage; raises StageError."""
    D = len(case["scale"])
    fail = lambda stage, msg: StageError(stage, f"{label or case.get('name', '')}: {msg}")
    B = scaled(case)
    nb = frobenius(B)
    tol = EPS * nb
    bad = not (np.isfinite(np.tril(case["mat"])).all() and np.isfinite(B).all() and np.isfinite(nb))
    if bad or res["status"] == 2:
        if not (bad and res["status"] == 2):
            raise fail("status", f"status {res['status']} for a matrix that is {'not ' if bad else ''}finite")
        for k in ("eig", "vec", "cov", "prec", "chol", "logdet", "off"):
            if not np.all(np.isnan(res[k])):
                raise fail("status", f"{k} is not NaN at status 2")
        if (res["n_low"], res["n_high"], res["sweeps_used"]) != (0, 0, 0):
            raise fail("status", "counts are not 0 at status 2")
        return {}
    worst = {}
    eig, vec = res["eig"], res["vec"]
    if not (np.isfinite(eig).all() and np.isfinite(vec).all()):
        raise fail("resid", "eig or vec is not finite")
    if np.any(np.diff(eig) < 0):
        raise fail("sorted", "eig is not ascending")
    if not 1 <= res["sweeps_used"] <= n_sweeps:
        raise fail("sweeps", f"sweeps_used = {res['sweeps_used']} is outside 1 .. {n_sweeps}")
    e = eigen_errors(res, case)
    worst["orth"] = _ratio(e["orth"], bars["orth"])
    worst["resid"] = _ratio(e["resid"], bars["resid"] * nb)
    if e["eig"] is not None:
        worst["eig"] = _ratio(e["eig"], bars["eig"] * nb)
    for k in ("orth", "resid", "eig"):
        if worst.get(k, 0.0) > 1.0:
            raise fail(k, f"{worst[k]:.3g} times its bar")
    _, n_low, n_high = clamp(eig, case)
    if (res["n_low"], res["n_high"]) != (n_low, n_high):
        raise fail("counts", f"(n_low, n_high) = {(res['n_low'], res['n_high'])}, the restatement has {(n_low, n_high)}")
    if not res["off"] >= 0:
        raise fail("status", "off is not a number")
    if res["off"] > tol or res["status"] == 3:
        if not (res["off"] > tol and res["status"] == 3):
            raise fail("status", f"status {res['status']} with off = {res['off']:.3g} and tol = {tol:.3g}")
        for k in ("cov", "prec", "chol", "logdet"):
            if not np.all(np.isnan(res[k])):
                raise fail("status", f"{k} is not NaN at status 3")
        return worst
    cov, prec, logdet, tc, tp, tl = matrices(eig, vec, case)
    fac = (D + 2) * EPS
    for k, want, terms in (("cov", cov, tc), ("prec", prec, tp), ("logdet", logdet, tl)):
        got = np.asarray(res[k])
        fin = np.isfinite(want)
        if not np.array_equal(np.isfinite(got), fin):
            raise fail(k, "its finite entries are not the restatement's")
        worst[k] = _ratio(np.abs(got - want)[fin], (fac * np.asarray(terms))[fin])
        if worst[k] > 1.0:
            raise fail(k, f"{worst[k]:.3g} times its bar")
        if got.ndim == 2 and not np.array_equal(got, got.T, equal_nan=True):
            raise fail(k, "not mirrored")
    own = np.asarray(res["cov"])
    want_chol = cholesky(own)
    if res["status"] == 1 or want_chol is None:
        if not (res["status"] == 1 and np.all(np.isnan(res["chol"]))):
            raise fail("chol", f"status {res['status']}; the restatement {'factors' if want_chol is not None else 'does not factor'} the result's cov")
        return worst
    if res["status"] != 0:
        raise fail("status", f"status {res['status']}")
    C = np.asarray(res["chol"])
    if not (np.isfinite(C).all() and np.all(np.triu(C, 1) == 0.0) and np.all(np.diag(C) > 0)):
        raise fail("chol", "not a lower factor")
    dg = np.sqrt(np.diag(own))
    worst["chol"] = _ratio(np.abs((C.astype(LD) @ C.T.astype(LD)).astype(np.float64) - own), (D + 1) * EPS * np.outer(dg, dg))
    if worst["chol"] > 1.0:
        raise fail("chol", f"{worst['chol']:.3g} times its bar")
    return worst


# ---- the test families ---------------------------------------------------------------------------------------------
SPECTRA = ("wide", "halfzero", "negative", "identity", "diagonal", "cov_zero")
DIMS = (1, 2, 3, 4, 5, 17, 48, 63, 64, 65)
ALL_SPECTRA_AT = (5, 17, 65)


def case_names():
    return [f"{s}_D{D}" for D in DIMS for s in SPECTRA if s == "wide" or D in ALL_SPECTRA_AT]


def _away(v, clamps):
    """the spectrum with every value within a factor 30 of a clamp moved a factor 30 further out"""
    v = np.array(v, dtype=np.float64)
    for c in clamps:
        near = (v > c / 30.0) & (v < c * 30.0)
        v[near] = np.where(v[near] < c, v[near] / 30.0, v[near] * 30.0)
    return v


def family(spectrum, D, seed=7):
    """the inputs of one case (no reference eigenvalues): a symmetric matrix with the given spectrum in prior units, behind
    random scales.  The exact cases (identity, diagonal) have scales that are powers of two."""
    rng = np.random.default_rng([seed, D, SPECTRA.index(spectrum)])
    q = np.linalg.qr(rng.standard_normal((D, D)))[0]
    kind, lam_lo, lam_hi = 0, 1.0, 2.0 ** 40
    s = 10.0 ** rng.uniform(-1.0, 1.0, D)
    if spectrum == "wide":
        e = _away(10.0 ** np.linspace(-14.0, 12.0, D) if D > 1 else [3e-5], (lam_lo,))
    elif spectrum == "halfzero":
        e = np.concatenate([np.zeros(D // 2), np.linspace(40.0, 900.0, D - D // 2)])
    elif spectrum == "negative":
        e = _away(np.linspace(-300.0, 500.0, D), (lam_lo,))
    elif spectrum in ("identity", "diagonal"):
        s = 2.0 ** rng.integers(-3, 4, D)
        e = np.ones(D) if spectrum == "identity" else rng.permutation(np.linspace(2.0, 100.0, D))
        q, lam_lo = np.eye(D), 0.5
    elif spectrum == "cov_zero":
        kind = 1
        e = np.concatenate([np.zeros(min(2, D - 1)), np.linspace(0.01, 0.2, D - min(2, D - 1))])
    else:
        raise ValueError(spectrum)
    b = (q * e[None, :]) @ q.T
    b = 0.5 * (b + b.T)
    mat = b / np.outer(s, s) if kind == 0 else b * np.outer(s, s)
    return make_case(mat, s, kind, lam_lo, lam_hi, name=f"{spectrum}_D{D}")


_golden = {}


def golden_cases():
    """{name: case} of the committed fixture: the families' inputs with their 40-digit eigenvalues"""
    if not _golden:
        g = np.load(GOLDEN, allow_pickle=False)
        for name in case_names():
            kind, lam_lo, lam_hi = g[name + "_par"]
            _golden[name] = make_case(g[name + "_mat"], g[name + "_scale"], int(kind), lam_lo, lam_hi, g[name + "_eig"], name)
    return _golden


_bars = {}


def golden_bars():
    """``measured_bars`` over the whole fixture, computed once"""
    if not _bars:
        _bars.update(measured_bars(list(golden_cases().values())))
    return _bars


def clamp_margin(case, bar_rel):
    """the smallest distance of a reference eigenvalue from a clamp (in eig's units), over the eig bar"""
    e = case["eig_ref"]
    lo, hi = case["lam_lo"], case["lam_hi"]
    edges = [lo, hi] if case["kind"] == 0 else [1.0 / lo, 1.0 / hi]
    edges = [c for c in edges if np.isfinite(c)]
    bar = bar_rel * frobenius(scaled(case))
    return min(float(np.min(np.abs(e - c))) for c in edges) / bar


def default_sweeps(cases):
    """the largest sweeps_used of the restatement over the cases, plus 4, capped at MAX_SWEEPS"""
    return min(MAX_SWEEPS, max(run(c, MAX_SWEEPS)["sweeps_used"] for c in cases) + 4)


# ---- duplicate lines: the Fisher information is singular ----------------------------------------------------------------
def duplicate_lines_case(n_lines=2, P=48):
    """a Voigt region whose first two lines have identical centre and widths and different amplitudes (``n_lines`` = 3: a
    third, separate line): the Jacobian's columns for c, L and G of the two are proportional, so the information has
    three null directions.  Returns (x, flux, noise, theta [4 n_lines])."""
    import fisher_ref
    x = np.arange(float(P)) - 0.5 * (P - 1)                 # a fit's device units: pixels from the region's middle
    lines = [(0.8, 1.5, 2.0, 4.0), (0.5, 1.5, 2.0, 4.0)] + ([(0.6, -12.0, 1.5, 3.0)] if n_lines == 3 else [])
    theta = np.array(lines, dtype=np.float64).ravel()
    noise = np.full(P, 0.05)
    flux = fisher_ref.jacobian(x, theta, len(lines), 1)[0] + noise * np.random.default_rng(3).standard_normal(P)
    return x, flux, noise, theta


# ---- a stand-in for the library -------------------------------------------------------------------------------------------
def fake_regularise(calls):
    """what tests put in place of ``vamp_amd.metric.regularise``: the restatement, every call recorded in ``calls``"""
    from vamp_amd import metric

    def regularise(mats, scales, kind="info", lam_lo=1.0, lam_hi=2.0 ** 40, n_sweeps=None, device=0, want=()):
        calls.append(dict(mats=mats, scales=scales, kind=kind, lam_lo=lam_lo, lam_hi=lam_hi, n_sweeps=n_sweeps))
        out = []
        for m, s in zip(mats, scales):
            m = np.asarray(m, dtype=np.float64)
            r = run(make_case(m, s, metric.KINDS[kind], lam_lo, lam_hi), n_sweeps or metric.DEFAULT_SWEEPS)
            out.append(metric.MetricRecord(**r))
        return out
    return regularise
