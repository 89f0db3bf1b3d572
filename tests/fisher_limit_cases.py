"""What the limit tests of libvamp_fisher.so share (tests/test_fisher_limits.py on the CPU, tests/test_gpu_fisher_limits.py
on the GPU, tests/golden/make_fisher_limits_golden.py): the case tables, the per-entry bars of the derivative evaluator,
the closure of the information matrix on a given Jacobian, the exact rational inverse of a given information matrix,
and the numpy copies of steps 4 to 6 of k_fisher in which the controls plant an error.

Per-entry bars.  An evaluator case is ONE Voigt line of G = 2 centred on 0: 1 / G is exact, so s = 2 sqrt(ln 2) / G,
y = L sqrt(ln 2) / G and u = x s are the same bits in numpy, in the host build and in the kernel, and the fixture holds
w = K + i M, w' and g = w + z w' at exactly those (u, y) (mpmath, 50 + 8 log10 |z| digits, rounded to fp64).  With
J_pd = -f pf_d Q_d, Q = (K, K_u, K + y K_y, K + u K_u + y K_y) and pf = (y sqrt(pi), -A y sqrt(pi) s, A sqrt(pi) s / 2,
-A y sqrt(pi) / G):
    |dJ_pd| <= b f |pf_d| S_d + eps (1 + tau) |J_pd|
    core (|z|^2 < 64), b = b_core: S = (K, S_Ku, S_TL, S_TL + |u| S_Ku), the sums of the identity's absolute terms,
        S_Ku = 2 (|u| K + y |M|), S_Ky = 2 (|u| |M| + y K) + 2 / sqrt(pi), S_TL = K + y S_Ky
    far, b = 32 eps: S = (|w|, |w'|, |g| + |u| |w'|, |g|), the moduli of the complex quantities whose real parts are taken
b_core = max(2 E_sc, 16 eps), E_sc the worst error over core scale of fisher_ref.jacobian (scipy's wofz and the identity)
on the same cases: reference against reference, measured by the generator and kept in the fixture."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np

import fisher_ref as ref

EPS = ref.EPS
SQRT_LN2 = 0.83255461115769775635          # the constant of lane_group.hpp's line_record
SQRT_PI = 1.7724538509055160273
FAR_B = 32 * EPS
R2_CORE = 64.0
NOISE = 0.05

# ---- 1. the evaluator's cases -------------------------------------------------------------------------------------------
A_EVAL, G_EVAL = 1.3, 2.0
Y_VALUES = (0.0, 1e-12, 5e-10, 2e-9, 1e-3, 0.5, 1.0, 2.0, 3.0, 5.0, 7.0, 7.9, 7.99, 8.0, 8.01, 8.1, 12.0, 30.0)
U_GRID = (0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 7.9, 8.5, 9.0, 10.0)
SEAM = 1e-3                                # pixel pairs at u^2 + y^2 = 64 (1 -+ SEAM)
U_WIDE = (0.5, 3.0, 7.0, 9.0, 20.0, 50.0, 100.0, 300.0, 1e3, 3e3, 1e4)
U_TAIL = tuple(np.round(np.linspace(0.3, 10.0, 32), 3))      # and one pixel at u = 11: 65 pixels, the last one alone in the second tile
G_HUGE = 2.0 ** -233                       # u = x 2 sqrt(ln 2) 2^233 = 2.3e70 x: beyond the 1e60 of voigt_grad_far's rescaling
X_HUGE = (1.5 * G_HUGE, 0.5, 1.0, 3.0)               # u = 2.5 (the core) and 1.2e70, 2.3e70, 6.9e70


def eval_name(y):
    return "eval_y%g" % y


EVAL_NAMES = tuple(eval_name(y) for y in Y_VALUES) + ("eval_wide_u", "eval_tail65", "eval_huge_z")


def line_uy(x, th):
    """(u [P], y, s) of a Voigt line as line_record and k_fisher form them (1 / G exact: G is a power of two here)"""
    _, c, L, G = th
    rG = 1.0 / G
    s = (2.0 * SQRT_LN2) * rG
    return (np.asarray(x, dtype=np.float64) - c) * s, (L * SQRT_LN2) * rG, s


def _L_for(y, G):
    """L with (L sqrt(ln 2)) / G == y exactly where a neighbour of y G / sqrt(ln 2) gives it, else the closest"""
    L = y * G / SQRT_LN2
    cand = [L]
    for _ in range(4):
        cand = [np.nextafter(cand[0], -np.inf)] + cand + [np.nextafter(cand[-1], np.inf)]
    return float(min(cand, key=lambda v: abs((v * SQRT_LN2) * (1.0 / G) - y))) if y > 0 else 0.0


def _symmetric_x(us, s):
    """no pixel at u = 0: M vanishes there, and with it the scale of K_u, while the trapezoid rule's M is a cancelling sum
    that leaves 1e-17 y in K_u -- nothing a bar made of the reference's own terms can hold (profiles/fisher_pointwise.txt)"""
    pos = np.array(sorted(set(float(u) for u in us))) / s
    return np.concatenate([-pos[::-1], pos])


def eval_inputs(name):
    """(x, theta) of an evaluator case"""
    if name == "eval_huge_z":
        x = _symmetric_x(X_HUGE, 1.0)
        return x, np.array([A_EVAL, 0.0, G_HUGE, G_HUGE])              # y = sqrt(ln 2)
    if name == "eval_wide_u":
        y, us = 1.0, list(U_WIDE)
    elif name == "eval_tail65":
        y, us = 0.5, list(U_TAIL)
    else:
        y = Y_VALUES[[eval_name(v) for v in Y_VALUES].index(name)]
        us = list(U_GRID)
        for sign in (-1.0, 1.0):
            r2 = 64.0 * (1.0 + sign * SEAM) - y * y
            if r2 > 0.0:
                us.append(math.sqrt(r2))
    th = np.array([A_EVAL, 0.0, _L_for(y, G_EVAL), G_EVAL])
    x = _symmetric_x(us, line_uy(0.0, th)[2])
    return (np.append(x, 11.0 / line_uy(0.0, th)[2]) if name == "eval_tail65" else x), th


def load_eval(path):
    """the evaluator cases of fisher_limits.npz: name, x, flux, noise, theta, u, y, s, w, wp, g (complex [P]), tau, jac [P, 4]"""
    g = np.load(path, allow_pickle=False)
    out = []
    for name in g["eval_cases"]:
        name = str(name)
        x, th, v = g[name + "_x"], g[name + "_theta"], g[name + "_ref"]
        u, y, s = line_uy(x, th)
        out.append({"name": name, "x": x, "flux": g[name + "_flux"], "noise": np.full(len(x), NOISE), "theta": th, "K": 1, "mode": 1,
                    "sd": False, "D": 4, "P": len(x), "u": u, "y": y, "s": s, "w": v[:, 0] + 1j * v[:, 1], "wp": v[:, 2] + 1j * v[:, 3],
                    "g": v[:, 4] + 1j * v[:, 5], "tau": v[:, 6], "jac": v[:, 7:11].copy()})
    return out, {"e_sc": float(g["eval_meta"][0]), "b_core": float(g["eval_meta"][1])}


def scipy_jacobian(c):
    """J [P, 4] of an evaluator case from scipy's wofz and the identity at the case's own (u, y): fisher_ref.jacobian's
    formulas at the bits the kernel sees (fisher_ref's sqrt(ln 2) is numpy's, an ulp from line_record's)"""
    from scipy.special import wofz
    u, y = c["u"], c["y"]
    w = wofz(u + 1j * y)
    K, M = w.real, w.imag
    Ku = -2.0 * (u * K - y * M)
    Ky = 2.0 * (u * M + y * K) - 2.0 / SQRT_PI
    Q = np.stack([K, Ku, K + y * Ky, K + u * Ku + y * Ky], axis=1)
    f = np.exp(-(c["theta"][0] * y * SQRT_PI * K))
    return -f[:, None] * prefactors(c)[None, :] * Q


def is_core(c):
    return c["u"] * c["u"] + c["y"] * c["y"] < R2_CORE


def prefactors(c):
    A, _, _, G = c["theta"]
    y, s = c["y"], c["s"]
    return np.array([y * SQRT_PI, -A * y * SQRT_PI * s, A * SQRT_PI * (0.5 * s), -(A * y * SQRT_PI) / G])


def entry_scales(c):
    """(core scales [P, 4], far scales [P, 4]) of Q = (K, K_u, K + y K_y, K + u K_u + y K_y)"""
    au, y = np.abs(c["u"]), c["y"]
    K, M = c["w"].real, np.abs(c["w"].imag)
    S_Ku = 2.0 * (au * K + y * M)
    S_TL = K + y * (2.0 * (au * M + y * K) + 2.0 / SQRT_PI)
    core = np.stack([K, S_Ku, S_TL, S_TL + au * S_Ku], axis=1)
    aw, awp, ag = np.abs(c["w"]), np.abs(c["wp"]), np.abs(c["g"])
    return core, np.stack([aw, awp, ag + au * awp, ag], axis=1)


def entry_bars(c, b_core):
    """(bar [P, 4] on J, core [P]): the per-entry bar of the module's docstring"""
    core_s, far_s = entry_scales(c)
    core = is_core(c)
    f = np.exp(-c["tau"])
    scale = np.where(core[:, None], b_core * core_s, FAR_B * far_s)
    return (f[:, None] * np.abs(prefactors(c))[None, :]) * scale + EPS * (1.0 + c["tau"])[:, None] * np.abs(c["jac"]), core


def ratio(err, bar):
    """error over bar entry by entry; a bar of 0 asks for equality"""
    with np.errstate(all="ignore"):
        return np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))


def entry_ratios(c, J, b_core):
    """worst error over bar of J's core entries and of its far entries (0.0 where the case has none)"""
    bar, core = entry_bars(c, b_core)
    r = ratio(np.abs(J - c["jac"]), bar)
    r = np.where(np.isnan(r), np.inf, r)
    return (float(r[core].max()) if core.any() else 0.0), (float(r[~core].max()) if (~core).any() else 0.0)


def host_lib():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "libvoigt_grad_host.so")
    if not os.path.exists(path):
        raise FileNotFoundError(path + " is not built: run __graft_entry__.build()")
    lib = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    for fn in (lib.voigt_grad_n, lib.voigt_grad_planted_n):
        fn.restype, fn.argtypes = None, [C.c_int, dp, dp, dp]
    return lib


def host_jacobian(lib, c, planted=False):
    """J [P, 4] of an evaluator case from the host build of voigt_grad.hpp, combined as fisher.hip combines it"""
    fn = lib.voigt_grad_planted_n if planted else lib.voigt_grad_n
    dp = C.POINTER(C.c_double)
    A, _, _, G = c["theta"]
    u, y, s = np.ascontiguousarray(c["u"]), c["y"], c["s"]
    yy, out = np.full_like(u, y), np.empty((u.size, 4))
    fn(u.size, u.ctypes.data_as(dp), yy.ctypes.data_as(dp), out.ctypes.data_as(dp))
    Ks, Ku, TL, TG = out.T
    r3 = A * y
    f = np.exp(-(r3 * Ks))
    a = np.stack([y * Ks, -(r3 * SQRT_PI) * s * Ku, (A * SQRT_PI) * (0.5 * s) * TL, -((r3 * SQRT_PI) / G) * TG], axis=1)
    return -f[:, None] * a


# ---- 2. the information matrix closed on a Jacobian ---------------------------------------------------------------------
def closure(jac, sigma, theta, K, mode, sd, with_prior=True, skip=()):
    """(sum [D, D], bar [D, D]): sum_p a_pi a_pj in np.longdouble with a_pd = fl(jac_pd * fl(1 / sigma_p)), the operations of
    k_fisher, and (P + 2) eps sum_p |a_pi a_pj| (+ 2 eps / A^2 and the prior's 1 / A^2 on amplitude diagonals); the free
    sd's row and column are left to the caller.  skip: pixels left out of the sum (the controls' planted error)"""
    P, D = jac.shape
    q = ref.q_of(mode)
    Dl = q * K
    a = (jac[:, :Dl] * (1.0 / np.asarray(sigma, dtype=np.float64))[:, None]).astype(np.longdouble)
    keep = np.ones(P, dtype=bool)
    keep[list(skip)] = False
    tot = np.einsum("pi,pj->ij", a[keep], a[keep])
    # (P 2^-1074: a product below the normal range, as in a Gaussian's wing, rounds to the subnormal grid in every fma)
    bar = (P + 2) * EPS * np.einsum("pi,pj->ij", np.abs(a), np.abs(a)).astype(np.float64) + P * 2.0 ** -1074
    if with_prior:
        for d in range(0, Dl, q):
            A = np.longdouble(theta[d])
            tot[d, d] += 1 / (A * A)
            bar[d, d] += 2 * EPS / float(theta[d]) ** 2
    return tot, bar


def closure_ratio(info, jac, sigma, theta, K, mode, sd, with_prior=True, skip=()):
    Dl = ref.q_of(mode) * K
    tot, bar = closure(jac, sigma, theta, K, mode, sd, with_prior, skip)
    return float(ratio(np.abs((info[:Dl, :Dl].astype(np.longdouble) - tot).astype(np.float64)), bar).max())


# ---- 3. dealing and factorisation edges ---------------------------------------------------------------------------------
# (name, mode, K, sd): P = Dl + 2 pixels; D = 64 is one lane per row with no second pass and no sd row, D = 61 and 49 the
# sd row behind 60 and 48 rows; the triangles of Dl = 24, 32, 45 have 300, 528 and 1035 entries (1, 2 and 4 full rounds of
# 256 threads and a partial one); K = 1, 3, 5 leave 3, 1 and 3 of the four line slots of a tile idle in the last round
DEALING = [("deal_voigt_K16", 1, 16, False), ("deal_voigt_K15_sd", 1, 15, True), ("deal_gauss_K16_sd", 0, 16, True),
           ("deal_gauss_K8", 0, 8, False), ("deal_voigt_K8", 1, 8, False), ("deal_gauss_K15", 0, 15, False)] + [
    ("deal_%s_K%d" % ("voigt" if m else "gauss", k), m, k, False) for m in (1, 0) for k in (1, 3, 5)]
# (name, mode, K, P).  P = 2 at K = 2 has D = 8 against rank <= 2 pixels + 2 priors: its information is singular whatever
# the lines are, so it is the one case of status 1 (J, grad and info compared; cov is NaN by definition)
PIXEL_EDGES = [("pixel_P2", 1, 2, 2), ("pixel_P128", 1, 2, 128), ("pixel_K5_P63", 1, 5, 63), ("pixel_K5_P64", 1, 5, 64),
               ("pixel_K5_P65", 1, 5, 65)]
TAIL_CASE = "pixel_K5_P65"                 # its last pixel is in every line's wing: the control of the closure test
OLD_CASES = ("H1215_r0_K4_m1_sd0_w0", "H1215_r0_K2_m1_sd1_w0", "CII1036_r1_K2_m0_sd0_w0", "pix_P129", "K16_voigt_sd", "K16_gauss",
             "far_line")                   # cases of fisher_cases.npz that the closure test also takes


def dealing_inputs(mode, K, sd):
    """(x, lines): lines spaced by 4 as in K16_voigt_sd of fisher_cases.npz, P = Dl + 2 pixels over them"""
    P = ref.q_of(mode) * K + 2
    x = np.linspace(-(2.0 * K + 2.0), 2.0 * K + 2.0, P)
    cen = [4.0 * (k - 0.5 * (K - 1)) for k in range(K)]
    if mode == 1:
        return x, [(0.4 + 0.05 * k, cen[k], 0.5 + 0.02 * k, 1.5 + 0.05 * k) for k in range(K)]
    return x, [(0.5 + 0.05 * k, cen[k], 1.2 + 0.03 * k) for k in range(K)]


def pixel_inputs(K, P):
    """(x, lines) of a PIXEL_EDGES case.  K = 5: narrow-damping lines (L = 2e-3) left of the centre, so that the last
    pixels lie about 20 Doppler widths from the nearest line"""
    if K == 2:
        x = np.linspace(-0.5 * P, 0.5 * P, P)
        w = max(P, 24) / 12.0
        return x, [(1.1, -1.5 * w, 0.4 * w, w), (0.7, 1.8 * w, 0.2 * w, 0.8 * w)]
    x = np.arange(P, dtype=np.float64) - 32.0
    return x, [(0.5 + 0.1 * k, -22.0 + 9.0 * k, 2e-3 * (1.0 + 0.1 * k), 1.5 + 0.05 * k) for k in range(5)]


# ---- 4. cov, sigma and logdet to the limit ------------------------------------------------------------------------------
# Rungs chosen with cholesky_copy on the CPU (tests/test_fisher_limits.py asserts it): the exact smallest pivot of the
# scaled matrix is >= 200 D eps on every rung but the last, which lies below D eps -- one rung in the undecided band.
# The Gaussian pair has kappa ~ 2e3 / delta^2 (the prior holds the amplitudes' difference); the Voigt pair's goes like
# delta^-4 (its L and G differences have no prior), so its ladder ends at larger delta.  It has no rung between 3e-3
# (kappa = 5e15) and its last: at delta = 1e-3 (kappa = 1e17) the eps-rounding of the information's own entries decides
# the sign of a leading minor -- the restatement's matrix has a smallest pivot of 4e3 D eps, the kernel's is indefinite
# in exact arithmetic -- so no reference made from the returned matrix can call such a rung decided.
DELTAS = {0: (3.0, 0.3, 0.03, 3e-3, 3e-4, 3e-5, 1e-5, 3e-7), 1: (3.0, 1.0, 0.3, 0.1, 0.03, 0.01, 3e-3, 3e-5)}
X40 = np.arange(40.0) - 19.5
# The Voigt pair lives on an abscissa of 2^32 units per pixel (a region in Hz has 3.7e9): u and y are the same bits as
# on the pixel scale, and the information of c, L and G is 2^-64 of it -- below D eps, which is what the status rule
# must not be applied to without scaling (the control)
UNIT = {0: 1.0, 1: 2.0 ** 32}
PIVOT_SAFE = 16.0                          # status must be 0 where the exact smallest pivot is at least PIVOT_SAFE D eps


def ladder(mode):
    """[(name, x, flux, noise, theta, K, mode)]: two lines of equal width 2.5 and amplitude 0.6 at 1.0 -+ 1.25 delta"""
    out, F = [], UNIT[mode]
    for d in DELTAS[mode]:
        line = (lambda c: (0.6, c * F, 1.0 * F, 2.5 * F)) if mode == 1 else (lambda c: (0.6, c, 2.5))
        th = np.array(line(1.0 - 1.25 * d) + line(1.0 + 1.25 * d))
        f, _ = ref.jacobian(X40 * F, th, 2, mode)
        flux = f + 0.04 * np.cos(1.7 * np.arange(40.0))
        out.append(("ladder_%s_%g" % ("voigt" if mode else "gauss", d), X40 * F, flux, np.full(40, 0.04), th, 2, mode))
    return out


def exact_stage(info):
    """Steps 4 to 6 of k_fisher in exact rational arithmetic on a given fp64 information matrix: a dict of cov (rounded
    to fp64), logdet, the smallest Cholesky pivot of the exactly scaled matrix C_ij = I_ij / sqrt(I_ii I_jj) (the pivots
    of I over its diagonal: scaling by a diagonal scales the pivots) and kappa, the 2-norm condition number of C from
    the exact inverse, and log_terms = sum |ln I_ii| + sum |ln pivot_i|, the absolute terms of the kernel's
    ln det I = sum ln I_ii + 2 sum ln L_ii; None where a leading minor is not positive"""
    D = info.shape[0]
    M = [[Fraction(float(info[i, j])) for j in range(D)] for i in range(D)]
    if any(M[i][i] <= 0 for i in range(D)):
        return None
    aug = [row[:] + [Fraction(int(i == j)) for j in range(D)] for i, row in enumerate(M)]
    piv = []
    for k in range(D):                       # elimination without pivoting: the pivots are those of L D L^T
        p = aug[k][k]
        if p <= 0:
            return None
        piv.append(p)
        for r in range(k + 1, D):
            m = aug[r][k] / p
            if m:
                aug[r] = [a - m * b for a, b in zip(aug[r], aug[k])]
    for k in range(D - 1, -1, -1):
        aug[k] = [a / aug[k][k] for a in aug[k]]
        for r in range(k):
            m = aug[r][k]
            if m:
                aug[r] = [a - m * b for a, b in zip(aug[r], aug[k])]
    cov = np.array([[float(aug[i][D + j]) for j in range(D)] for i in range(D)])
    logs = [math.log(float(p)) for p in piv]                 # a pivot lies between its diagonal entry and the matrix's smallest eigenvalue
    scaled = [float(p / M[k][k]) for k, p in enumerate(piv)]
    d = np.sqrt(np.diag(info))
    Cs, Ci = info / np.outer(d, d), cov * np.outer(d, d)
    return {"cov": cov, "logdet": math.fsum(logs), "min_pivot": min(scaled), "kappa": float(np.linalg.norm(Cs, 2) * np.linalg.norm(Ci, 2)),
            "log_terms": float(np.sum(np.abs(np.log(np.diag(info)))) + sum(abs(math.log(v)) for v in scaled))}


def cholesky_copy(info, scale=True, rule=True):
    """numpy copy of steps 4 to 6 of k_fisher: (cov, logdet, status).  scale = False factorises the matrix as it is,
    rule = False accepts every positive pivot instead of those above D eps"""
    D = info.shape[0]
    dg = np.diag(info).copy()
    sq = np.sqrt(dg) if scale else np.ones(D)
    a = info / np.outer(sq, sq)
    ok = bool(np.all((dg > 0) & np.isfinite(dg)))
    thr = D * EPS
    with np.errstate(all="ignore"):
        for k in range(D):
            piv = a[k, k]
            if not piv > (thr if rule else 0.0):
                ok, piv = False, 1.0
            l = np.sqrt(piv)
            a[k + 1:, k] *= 1.0 / l
            a[k, k] = l
            for r in range(k + 1, D):
                a[r, k + 1:r + 1] -= a[r, k] * a[k + 1:r + 1, k]
        Lm = np.tril(a)
        X = np.zeros((D, D))
        for j in range(D):
            X[j, j] = 1.0 / Lm[j, j]
            for i in range(j + 1, D):
                X[i, j] = -(Lm[i, j:i] @ X[j:i, j]) / Lm[i, i]
        cov = (X.T @ X) / np.outer(sq, sq)
        logdet = float(np.sum(np.log(dg)) + 2.0 * np.sum(np.log(np.diag(Lm)))) if scale else float(2.0 * np.sum(np.log(np.diag(Lm))))
    if not ok:
        return np.full((D, D), np.nan), float("nan"), 1
    return np.tril(cov) + np.tril(cov, -1).T, logdet, 0


def stage_ratios(cov, logdet, ex):
    """error over kappa eps of a covariance (entry by entry against sqrt(S_ii S_jj)) and of a ln det: the bar is D"""
    s = np.sqrt(np.diag(ex["cov"]))
    ke = ex["kappa"] * EPS
    return float(np.max(np.abs(cov - ex["cov"]) / np.outer(s, s))) / ke, abs(logdet - ex["logdet"]) / ke
