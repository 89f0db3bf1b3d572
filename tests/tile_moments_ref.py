"""numpy restatement of the moment form of a far-field-only tile's chi^2 (helper, not a test module).

A full 256-pixel tile without a near line has a model flux m = exp(-tau) whose optical depth is the tile's interpolant and
nothing else.  With a = 1 - m its chi^2 is

    sum w^2 ((f - 1) + a)^2 = C0 + 2 b.S + b'Qb,      a = sum_j b_q[j] u^j on quarter q of the tile,

where the moments S_q[j] = sum w^2 (f - 1) u^j, Q_q[n] = sum w^2 u^n and C0 = sum w^2 (f - 1)^2 belong to the data alone.
The moment form interpolates the ABSORPTION through the tile's 16 Chebyshev nodes (a_n = -expm1(-tau_n)); the per-pixel form
interpolates the optical depth and takes the exponential at each pixel.

Everything here follows the kernels' definitions: the transform is vamp_amd/csrc/ff_matrix.inc, the tile geometry and the
pixels' places u are k_tile_tables', the classification is ff_classify_batch's, the guard is ff_moments_ok's
(vamp_amd/csrc/ff_moments.hpp).  Quarters are indexed in coefficient order (ascending x), so a descending grid gives the
same moments as its mirror image.
"""
import os
import re

import numpy as np

TILE, NODES, DEG, ROWS = 256, 16, 13, 56
NS, NQ = DEG + 1, 2 * DEG + 1                      # moments per quarter: S_q[0..13], Q_q[0..26]
R2_CORE, FF_DIST, WIDE_MAX, MID_Z2 = 64.0, 2.0, 0.75, 30.25
SQRT_LN2 = np.sqrt(np.log(2.0))
GUARD_ULPS = 8.0                                   # rounding of the moment form: GUARD_ULPS 2^-53 M
GUARD_BOUND = 2.0 ** -40 * TILE                    # ... may be at most this (1e-12 of a fitted tile's own chi^2)
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ff_matrix():
    """(M[56, 16], nodes[16]) of vamp_amd/csrc/ff_matrix.inc; row 14 q + j, layout [n/2][row][n%2]"""
    txt = open(os.path.join(_ROOT, "vamp_amd", "csrc", "ff_matrix.inc")).read()
    body = txt[txt.index("{", txt.index("FF_M[")) + 1:txt.rindex("}")]
    body = re.sub(r"//[^\n]*", "", body)
    v = np.array([float(s) for s in body.replace("\n", " ").split(",") if s.strip()])
    assert v.size == ROWS * NODES + NODES
    M = v[:ROWS * NODES].reshape(NODES // 2, ROWS, 2).transpose(1, 0, 2).reshape(ROWS, NODES)
    return M, v[ROWS * NODES:]


def tile_geometry(x):
    """k_tile_tables on the host: (mid[nt], half[nt], up, u[nt, 256], quarter[256]) of a region's full tiles"""
    nt = x.size // TILE
    xt = x[:nt * TILE].reshape(nt, TILE)
    lo, hi = xt[:, 0], xt[:, -1]
    mid, half = 0.5 * (lo + hi), 0.5 * np.abs(hi - lo)
    up = bool(hi[0] > lo[0])
    t = np.arange(TILE) >> 6
    q = t if up else 3 - t
    u = (xt - (half[:, None] * (0.5 * q - 0.75)[None, :] + mid[:, None])) * (4.0 / half)[:, None]
    return mid, half, up, u, q


def tile_moments(x, flux, noise, dtype=np.float64):
    """(S[nt, 4, 14], Q[nt, 4, 27], C0[nt]) of the full tiles, quarters in coefficient order"""
    mid, half, up, u, q = tile_geometry(x)
    nt = mid.size
    w2 = (1.0 / noise[:nt * TILE].reshape(nt, TILE).astype(dtype)) ** 2
    d = flux[:nt * TILE].reshape(nt, TILE).astype(dtype) - 1
    u = u.astype(dtype)
    S, Q = np.zeros((nt, 4, NS), dtype), np.zeros((nt, 4, NQ), dtype)
    for qq in range(4):
        sel = q == qq
        pw = np.ones_like(u[:, sel])
        for n in range(NQ):
            Q[:, qq, n] = (w2[:, sel] * pw).sum(axis=1)
            if n < NS:
                S[:, qq, n] = (w2[:, sel] * d[:, sel] * pw).sum(axis=1)
            pw = pw * u[:, sel]
    return S, Q, (w2 * d * d).sum(axis=1)


def guard_ok(C0, Q0sum, amax):
    """the tile may take the moment path: rounding bound 8 2^-53 (sqrt C0 + amax sqrt sum_q Q_q[0])^2 <= 2^-40 256"""
    r = np.sqrt(C0) + amax * np.sqrt(Q0sum)
    return GUARD_ULPS * 2.0 ** -53 * (r * r) <= GUARD_BOUND


def guard_try(C0, Q0sum):
    """asked before the node stage, of the data alone (vamp::ff_moments_try): guard_ok with amax = 0, and 2 sqrt C0 <= 2^9 --
    where the model fits, sqrt(C0 / sum Q_q[0]) is the tile's r.m.s. absorption, which amax cannot be below"""
    return guard_ok(C0, Q0sum, 0.0) & (2.0 * np.sqrt(C0) <= 512.0)


def chi2_moments(b, S, Q, C0):
    """chi^2 of one tile from b[4, 14] as the lanes form it: sum_{q,j} b_q[j] (sum_l b_q[l] Q_q[j+l] + 2 S_q[j]) + C0"""
    b = np.asarray(b)
    chi = b.dtype.type(0)
    for q in range(4):
        for j in range(NS):
            chi = chi + b[q, j] * (np.dot(b[q], Q[q, j:j + NS]) + 2 * S[q, j])
    return chi + C0


def chi2_direct(b, u, q, flux, noise):
    """the same sum pixel by pixel: sum w^2 ((f - 1) + a(u))^2 with a on each quarter from b"""
    b = np.asarray(b)
    a = np.zeros(u.shape, b.dtype)
    for j in range(DEG, -1, -1):
        a = a * u + b[q, j]
    return ((((flux - 1) + a) / noise) ** 2).sum()


def classify(native, x):
    """ff_classify_batch: (far, wide, near)[W, K, nt] from native[W, K, 4] = (A, c, L, G)"""
    mid, half = tile_geometry(x)[:2]
    cc, L, G = native[:, :, 1], native[:, :, 2], native[:, :, 3]
    s, y = 2.0 * SQRT_LN2 / G, L * SQRT_LN2 / G
    w8 = np.sqrt(np.maximum(R2_CORE - y * y, 0.0)) / s
    wmid = np.sqrt(np.maximum(MID_Z2 - y * y, 0.0)) / s
    dist = np.abs(mid[None, None, :] - cc[:, :, None]) - half[None, None, :]
    away = dist >= FF_DIST * half[None, None, :]
    far = away & (dist >= w8[:, :, None])
    wide = ((s * (0.5 * 2.0 * half.max()) <= WIDE_MAX)[:, :, None] | (away & (dist >= wmid[:, :, None]))) & ~far
    return far, wide, ~(far | wide)


def voigt_tau(x, native):
    """[K', n] optical depths of lines native[K', 4] at x[n] (the oracle's voigt_function)"""
    from scipy.special import wofz
    A, c, L, G = [native[:, i][:, None] for i in range(4)]
    z = (2.0 * (x[None, :] - c) + 1j * L) * SQRT_LN2 / G
    return A * L * np.sqrt(np.pi) * SQRT_LN2 / G * wofz(z).real


def walker_tiles(native, x, flux, noise, moments=None, M=None):
    """One walker (native[K, 4]) against the exact sum, tile by tile.  Returns a dict of arrays over the full tiles:
    exact, pixel (optical depth interpolated, exp per pixel: the per-pixel form), moment (moment form where the tile
    qualifies, else = pixel), takes (no near line and the guard holds), nonear, amax."""
    if M is None:
        M = ff_matrix()
    Mat, nodes = M
    mid, half, up, u, q = tile_geometry(x)
    nt = mid.size
    S, Q, C0 = moments if moments is not None else tile_moments(x, flux, noise)
    far, wide, near = [m[0] for m in classify(native[None], x)]
    tau_all = voigt_tau(x[:nt * TILE], native).reshape(native.shape[0], nt, TILE)
    out = {k: np.zeros(nt) for k in ("exact", "pixel", "moment", "amax")}
    out["takes"], out["nonear"] = np.zeros(nt, bool), np.zeros(nt, bool)
    for i in range(nt):
        sl = slice(i * TILE, (i + 1) * TILE)
        f, sd = flux[sl], noise[sl]
        interp = far[:, i] | wide[:, i]
        tau_near = tau_all[near[:, i], i].sum(axis=0)
        out["exact"][i] = (((f - np.exp(-tau_all[:, i].sum(axis=0))) / sd) ** 2).sum()
        taun = voigt_tau(mid[i] + half[i] * nodes, native[interp]).sum(axis=0) if interp.any() else np.zeros(NODES)
        coef = (Mat @ taun).reshape(4, NS)
        tau_ff = np.zeros(TILE)
        for j in range(DEG, -1, -1):
            tau_ff = tau_ff * u[i] + coef[q, j]
        out["pixel"][i] = (((f - np.exp(-(tau_near + tau_ff))) / sd) ** 2).sum()
        out["moment"][i] = out["pixel"][i]
        out["nonear"][i] = not near[:, i].any()
        if out["nonear"][i]:
            an = -np.expm1(-taun)
            out["amax"][i] = np.abs(an).max()
            if guard_try(C0[i], Q[i, :, 0].sum()) and guard_ok(C0[i], Q[i, :, 0].sum(), out["amax"][i]):
                out["takes"][i] = True
                out["moment"][i] = chi2_moments((Mat @ an).reshape(4, NS), S[i], Q[i], C0[i])
    return out
