"""Zero-residual regions: a per-pixel bound on the flux error of the chi^2 sweep (helper, not collected by pytest).

The data of a case IS the oracle's model flux f*_i = vo.model_flux(region, theta*), without noise, and the noise is a
per-pixel allowance sigma_i.  At any walker whose exact model is f*, the chi^2 a kernel returns is
sum_i ((f*_i - m_i) / sigma_i)^2 >= max_i ((f*_i - m_i) / sigma_i)^2, so chi^2 <= 1 proves that EVERY pixel's model
flux is within its allowance: quadratic in the error, no cancellation between pixels, no dependence on residuals.  The
oracle's chi^2 is identically 0 and costs one evaluation per region, so the check runs at production walker counts.

Walkers that differ but share the exact model (walker_family):
  * permutations of the truth's components;
  * amplitude splits of coincident components: lines k, k' with one centre and widths carry s A and (1 - s) A
    (tau is linear in the amplitude, in N for (N, b, z)); stretch moves are affine, so a split-only ensemble's every
    proposal is again a zero-residual point (the sampler test checks every stored lnprob);
  * free-sd mode: the returned chi^2 is the unweighted sum (f - m)^2, an absolute bound; walkers differ in sd.

The allowance (ALLOWANCE) is derived from DESIGN.md's error statements, not measured:
  sigma_i = eps_abs + f*_i (eps_rel max_{|j - i| < TILE} tau*_j + eps_ctr sum_k tau_k^peak)
            [+ fp32: f*_i sum_k |d tau_k / dx| dx_i]
with tau*_j the oracle's optical depth at pixel j (its largest value over any tile that holds pixel i: tile_max) and
tau_k^peak line k's optical depth at its own centre.
"""
import dataclasses
import math

import numpy as np

from oracle import vamp_oracle as vo

TILE = 256                    # pixels per tile of the long-region sweep
U32 = 2.0 ** -24              # unit roundoff of fp32
NARROW_PX = 1e-3              # fp32 cannot resolve a Gaussian width below this (tests/test_gpu_fp32.py): no such line in
                              # an fp32 case (make_case refuses them); the fp64 cases go down to it

# (eps_abs, eps_rel, eps_ctr) per dtype, each from a DESIGN.md statement:
#   fp64  eps_abs 1e-14: the far-field sweep's model flux is exp(-tau) by the degree-11 kernel, 6e-15 of a flux <= 1
#                        (VAMP_FLUX_EXP_DROP), plus the oracle's own rounding of exp;
#         eps_rel 1e-10: the far field reproduces a wing from 2 half-widths to 3e-11 of its own value (section 3,
#                        test_ff_matrix.py), the device and scipy's wofz to 1e-13 (section 6), times 3 for the lines
#                        between far and near and the tile interpolant of lines wider than a tile, which share it;
#         eps_ctr 1e-15: the per-line Taylor tables have absolute error <= 3e-16 of the line centre (section 3), for
#                        each line whose table covers the pixel; x3 for the sum over the tables in reach.
#   fp32  eps_abs 3e-7:  the data (and the noise) are stored in fp32 (vamp_set_regions' fp32 copies): f* rounded to
#                        fp32 moves it by <= 6e-8, and exp(-tau) by the fp32 exp costs a few ulp of m <= 1;
#         eps_rel 2e-4:  Humlicek W4's relative error <= 7.6e-5 (section 6), the 8-node far field 2.6e-7,
#                        tau summed over <= 16 lines in fp32 (16 ulp), x2;
#         eps_ctr 2e-7:  the fp32 Taylor rows have absolute error <= 6.5e-8 of the line centre (section 3), x3;
#         and a term of its own, dx: the fp32 context evaluates |x_i - c_k| from x and c rounded to fp32, an
#                        abscissa error <= U32 (|x_i| + |c_k| + |x_i - c_k|); it moves tau by |d tau_k / dx| times that,
#                        bounded here by the oracle's own tau at x_i +- 2 U32 (|x_i| + max_k |c_k|).
#   fp32  x sqrt(P): chi^2 <= 1 follows from per-pixel bounds E_i only if sigma_i >= sqrt(P) E_i.  The fp64 errors are
#                        concentrated (tables, interpolants) and pass without it; the fp32 ones are rounding-level at
#                        EVERY pixel (fp32 data, x and exp), and their sum over a long region exceeds 1 by itself.
ALLOWANCE = {"f64": (1e-14, 1e-10, 1e-15), "f32": (3e-7, 2e-4, 2e-7)}
# lnprob == prior - chi^2 / 2 (+ the sd term) to this relative tolerance: fp64 to rounding; the fp32 context's sum
# carries fp32-rounded terms (measured up to 1e-8 of |lnprob|), the fp32 bar on lnprob is 1e-3 (test_gpu_fp32.py)
LNP_IDENTITY = {"f64": 1e-10, "f32": 1e-6}
HUGE_NOISE = 1e30             # localisation: the noise outside the tile under test


@dataclasses.dataclass
class Case:
    name: str
    region: vo.Region          # flux = f*, noise = sigma, explicit bounds
    truth: np.ndarray          # theta* [D]
    tau: np.ndarray            # tau*_i
    sigma: np.ndarray          # the allowance
    dtype: str
    nbz: np.ndarray = None     # [4] row of set_regions' nbz, or None
    splits: tuple = ()         # ((k, k'), ...) coincident pairs of the truth (amplitude index q k, q k')

    @property
    def bounds(self):
        r = self.region
        return np.array([r.c_lo, r.c_hi, r.sigma_max, r.fwhm_max])


def _centres(region, theta):
    with np.errstate(all="ignore"):
        return np.array([comp[1] for comp in vo.native_components(region, theta)])


def line_peaks(region, theta):
    """tau_k at line k's own centre"""
    c = _centres(region, theta)
    at = dataclasses.replace(region, x=c, flux=np.ones(c.size), noise=np.ones(c.size))
    return np.diag(vo.component_taus(at, theta)).copy()


def tile_max(v):
    """max of v over the pixels within TILE - 1 of each pixel: the interpolants and tables of the sweep are accurate
    relative to what they reproduce over a whole tile (Chebyshev interpolation error is a sup-norm statement), so a
    pixel's error may be a fraction of the largest tau of any tile it shares, not of its own tau"""
    from numpy.lib.stride_tricks import sliding_window_view
    pad = np.concatenate([np.full(TILE - 1, -np.inf), v, np.full(TILE - 1, -np.inf)])
    return sliding_window_view(pad, 2 * TILE - 1).max(axis=1)


def make_case(name, x, truth, K, mode=vo.MODE_VOIGT4, dtype="f64", nbz=None, sample_sd=False, splits=(), pad=0.0,
              data_shift=None, probe_tile=None):
    """One zero-residual region.  ``pad``: the centre bounds widened by this much beyond the grid (lines centred off the
    grid); ``nbz``: [l_fixed, line, x_origin, x_scale].  ``data_shift``: added to f* after the allowance is built (the
    negative controls).  ``probe_tile`` (the probe cases of tests/ff_visibility.py only): the check is localised to that
    tile -- HUGE_NOISE at every other pixel -- and the allowance inside it is the one derived above with its two global
    terms made local, never larger than the default one: eps_ctr counts only the lines whose Taylor table covers the
    pixel (|z|^2 < 64, as the comment above ALLOWANCE says), and the fp32 factor is sqrt(TILE), the pixels the check
    sums over, instead of sqrt(P)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    P = x.size
    lo, hi = float(x.min()), float(x.max())
    sigma_max = (hi - lo) / 2.0
    kw = dict(c_lo=lo - pad, c_hi=hi + pad, sigma_max=sigma_max, fwhm_max=sigma_max * vo.FWHM_PER_SIGMA)
    if nbz is not None:
        kw.update(l_fixed=float(nbz[0]), line=float(nbz[1]), x_origin=float(nbz[2]), x_scale=float(nbz[3]))
    truth = np.asarray(truth, dtype=np.float64).ravel()
    r0 = vo.Region(x=x, flux=np.ones(P), noise=np.ones(P), n_comp=K, mode=mode, sample_sd=sample_sd, **kw)
    taus = vo.component_taus(r0, truth)
    tau = sum(list(taus))                              # model_flux's own order
    f = vo.model_flux(r0, truth)
    assert np.all(np.isfinite(f)) and np.isfinite(vo.log_prior(r0, np.append(truth, 0.5) if sample_sd else truth)), name
    eps_abs, eps_rel, eps_ctr = ALLOWANCE[dtype]
    peaks = line_peaks(r0, truth)
    ctr = peaks.sum()
    if probe_tile is not None:
        assert mode == vo.MODE_VOIGT4 and not sample_sd, name
        t4 = truth.reshape(K, 4)
        s_k, y_k = 2.0 * vo.SQRT_LN2 / t4[:, 3], t4[:, 2] * vo.SQRT_LN2 / t4[:, 3]
        covers = np.abs(x[None, :] - t4[:, 1, None]) * s_k[:, None] < np.sqrt(np.maximum(64.0 - y_k ** 2, 0.0))[:, None]
        ctr = (peaks[:, None] * covers).sum(0)
    sigma = eps_abs + f * (eps_rel * tile_max(tau) + eps_ctr * ctr)
    if dtype == "f32":
        comps = vo.native_components(r0, truth)
        px = np.median(np.abs(np.diff(x))) if P > 1 else 1.0
        widths = [abs(c[2]) if mode == vo.MODE_GAUSS3 else abs(c[3]) for c in comps]
        assert min(widths) > NARROW_PX * px, (name, "fp32 case with a line narrower than NARROW_PX", min(widths))
        h = 2.0 * U32 * (np.abs(x) + np.abs(_centres(r0, truth)).max())
        slope = np.zeros(P)
        for s in (1.0, -1.0):
            rs = dataclasses.replace(r0, x=x + s * h)
            slope = np.maximum(slope, np.abs(vo.component_taus(rs, truth) - taus).sum(0))
        sigma = (sigma + f * slope) * math.sqrt(P if probe_tile is None else min(P, TILE))
    if probe_tile is not None:
        inside = np.arange(P) // TILE == probe_tile
        assert inside.any(), (name, probe_tile)
        sigma = np.where(inside, sigma, HUGE_NOISE)
    flux = f if data_shift is None else f + data_shift(sigma)
    region = dataclasses.replace(r0, flux=flux, noise=sigma)
    return Case(name, region, truth, tau, sigma, dtype, None if nbz is None else np.asarray(nbz, dtype=np.float64),
                tuple(splits))


def with_split(comps, k, s=0.5):
    """[K, q] -> [K + 1, q]: line k split into s A and (1 - s) A, the new line appended"""
    comps = np.array(comps, dtype=np.float64)
    dup = comps[k].copy()
    dup[0] = (1.0 - s) * comps[k, 0]
    comps[k, 0] = s * comps[k, 0]
    return np.vstack([comps, dup[None, :]]), (k, comps.shape[0])


def walker_family(case, W, rng, permute=True, split=True, sd=None):
    """W walkers with the truth's exact model: components permuted (per walker), every coincident pair's amplitude
    split anew (s ~ U(0.05, 0.95)), and a free sd ~ U(sd) appended in sample_sd mode.  Walker 0 is the truth."""
    r = case.region
    q, K = r.q, r.n_comp
    comps = np.broadcast_to(case.truth[:q * K].reshape(K, q), (W, K, q)).copy()
    if split:
        for k, k2 in case.splits:
            total = comps[:, k, 0] + comps[:, k2, 0]
            s = rng.uniform(0.05, 0.95, W)
            comps[:, k, 0], comps[:, k2, 0] = s * total, (1.0 - s) * total
    if permute and K > 1:
        perm = rng.random((W, K)).argsort(axis=1)
        comps = np.take_along_axis(comps, perm[:, :, None], axis=1)
    comps[0] = case.truth[:q * K].reshape(K, q)
    th = comps.reshape(W, q * K)
    if r.sample_sd:
        lo, hi = sd if sd is not None else (0.01, 0.9)
        th = np.hstack([th, rng.uniform(lo, hi, (W, 1))])
    return np.ascontiguousarray(th)


def log_prior_batch(region, th):
    """vo.log_prior over the rows of th (the same operations in the same order, vectorised over walkers)"""
    th = np.asarray(th, dtype=np.float64)
    W, q, K = th.shape[0], region.q, region.n_comp
    t = th[:, :q * K].reshape(W, K, q)
    lp = np.zeros(W)

    def xexp(v):
        with np.errstate(all="ignore"):
            return np.where((v < 0) | ~np.isfinite(v), -np.inf, np.log(v * np.exp(-v)))

    def unif(v, lo, hi):
        return np.where((v >= lo) & (v <= hi), -math.log(hi - lo), -np.inf)

    with np.errstate(all="ignore"):
        for k in range(K):
            if region.mode == vo.MODE_GAUSS3:
                a, c, s = t[:, k, 0], t[:, k, 1], t[:, k, 2]
                lp = lp + xexp(a) + 0.0
                lp = lp + unif(c, region.c_lo, region.c_hi)
                lp = lp + unif(s, 0.0, region.sigma_max)
            elif region.mode == vo.MODE_VOIGT4:
                a, c, L, G = t[:, k, 0], t[:, k, 1], t[:, k, 2], t[:, k, 3]
                lp = lp + xexp(a)
                lp = lp + unif(c, region.c_lo, region.c_hi)
                lp = lp + unif(L, 0.0, region.fwhm_max)
                lp = lp + unif(G, 0.0, region.fwhm_max)
            else:
                amp, nu_c, sig = vo.nbz_to_native(t[:, k, 0], t[:, k, 1], t[:, k, 2], region.line)
                c = (nu_c - region.x_origin) / region.x_scale
                G = (sig / region.x_scale) * vo.FWHM_PER_SIGMA
                lp = lp + xexp(amp)
                lp = lp + unif(c, region.c_lo, region.c_hi)
                lp = lp + unif(G, 0.0, region.fwhm_max)
        if region.sample_sd:
            lp = lp + unif(th[:, -1], 0.0, 1.0)
    return lp


def set_cases(ctx, cases):
    """upload the cases as the regions of ctx (one mode / sd for all)"""
    r0 = cases[0].region
    assert all(c.region.mode == r0.mode and c.region.sample_sd == r0.sample_sd for c in cases)
    nbz = np.array([c.nbz for c in cases]) if r0.mode == vo.MODE_NBZ3 else None
    ctx.set_regions([c.region.x for c in cases], [c.region.flux for c in cases], [c.region.noise for c in cases],
                    [c.region.n_comp for c in cases], mode=r0.mode, sample_sd=r0.sample_sd,
                    bounds=np.array([c.bounds for c in cases]), nbz=nbz)


def normalised(case, chi):
    """sqrt(chi^2) in units of the allowance: known noise -> per-pixel (chi^2 is weighted by 1/sigma_i^2);
    free sd -> the unweighted sqrt(sum (f - m)^2) over the largest sigma_i (an absolute bound)"""
    chi = np.asarray(chi, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        if case.region.sample_sd:
            return np.sqrt(chi) / case.sigma.max()
        return np.sqrt(chi)


def verdict(case, th, lnp, chi):
    """(worst normalised error, list of problems) of one region's walkers"""
    prior = log_prior_batch(case.region, th)
    fin = np.isfinite(prior)
    problems = []
    if not np.array_equal(fin, np.isfinite(lnp)):
        problems.append("finite / -inf pattern differs from the prior's at walkers %s" % np.flatnonzero(fin != np.isfinite(lnp))[:8])
    fin &= np.isfinite(lnp)
    e = normalised(case, chi[fin])
    worst = float(np.max(np.where(np.isnan(e), np.inf, e), initial=0.0))
    bad = np.flatnonzero(fin)[~(e <= 1.0)]
    if bad.size:
        problems.append("%d walkers beyond the allowance, worst sqrt(chi2) %.3g at walker %d" % (bad.size, worst, bad[np.argmax(e[~(e <= 1.0)])]))
    r = case.region
    if r.sample_sd:
        sd = th[fin, -1]
        ll = r.x.size * 0.5 * np.log(1.0 / sd ** 2 / (2.0 * math.pi)) - 0.5 * chi[fin] / sd ** 2
    else:
        ll = -0.5 * chi[fin] + r.norm_const
    err = np.abs(lnp[fin] - (prior[fin] + ll)) / np.maximum(1.0, np.abs(lnp[fin]))
    if err.size and err.max() > LNP_IDENTITY[case.dtype]:
        problems.append("lnprob != prior - chi2 / 2 by %.3g at walker %d" % (err.max(), np.flatnonzero(fin)[np.argmax(err)]))
    return worst, problems, bad


def localise(ctx, case, th_bad):
    """Which tile: the failing walkers through copies of the region, each with noise HUGE_NOISE outside one tile.
    Returns (chi2 [tiles, walkers], index of the worst tile of the worst walker).  Replaces ctx's regions."""
    x, P = case.region.x, case.region.x.size
    T = (P + TILE - 1) // TILE
    copies = []
    for t in range(T):
        n = np.full(P, HUGE_NOISE)
        n[t * TILE:(t + 1) * TILE] = case.sigma[t * TILE:(t + 1) * TILE]
        copies.append(dataclasses.replace(case, region=dataclasses.replace(case.region, noise=n)))
    set_cases(ctx, copies)
    th_bad = np.atleast_2d(th_bad)
    if th_bad.shape[0] % 2:
        th_bad = np.vstack([th_bad, th_bad[-1:]])
    _, chi = ctx.lnprob_all([th_bad] * T, return_chi2=True)
    w = int(np.nanargmax(np.nanmax(chi, axis=0)))
    return chi, int(np.nanargmax(chi[:, w]))


def check(ctx, cases, thetas, label, report=None, localise_on_failure=True):
    """One lnprob_all over the regions of ctx (== cases, in order): every walker within its allowance, the finite /
    -inf pattern of the prior, lnprob = prior - chi^2 / 2.  On failure the message names the case, the walker, the
    tile and its pixels (a second launch over one copy of the region per tile; free-sd regions are not localised).
    Returns {case name: worst normalised error}."""
    lnp, chi = ctx.lnprob_all(thetas, return_chi2=True)
    out, failures = {}, []
    for r, case in enumerate(cases):
        worst, problems, bad = verdict(case, thetas[r], lnp[r], chi[r])
        out[case.name] = worst
        if problems:
            failures.append((case, r, problems, bad))
    if report is not None:
        report.update(out)
    if failures:
        msgs = []
        for case, r, problems, bad in failures:
            msg = "%s / %s: %s" % (label, case.name, "; ".join(problems))
            if localise_on_failure and bad.size and not case.region.sample_sd:
                worst = bad[np.argsort(-chi[r][bad])[:4]]
                tchi, tile = localise(ctx, case, thetas[r][worst])
                msg += "; worst walker %d: tile %d, pixels [%d, %d), sqrt(chi2) of that tile %.3g" % (
                    worst[0], tile, tile * TILE, min(case.region.x.size, (tile + 1) * TILE), math.sqrt(tchi[tile, 0]))
                localise_on_failure = False            # ctx now holds the copies
            msgs.append(msg)
        raise AssertionError("\n".join(msgs))
    return out


def print_report(label, report):
    for name, v in report.items():
        print("zero-residual %s / %s: worst sqrt(chi2) %.3g" % (label, name, v))


# -- case builders -------------------------------------------------------------------------------------------------
def amp_for_peak(L, G, peak):
    """Voigt1D amplitude whose profile peaks at ``peak`` (clipped into the xexp prior's finite range)"""
    unit = vo.voigt_function(np.zeros(np.size(L)), 0.0, 1.0, np.asarray(L, dtype=np.float64), np.asarray(G, dtype=np.float64))
    return np.clip(peak / unit, 1e-6, 500.0)


def headline_truth(P=16384, K=16, seed=20240517):
    """bench.make_workload's truth (NBZ3) and the nbz row: the same draws, without the walkers' perturbation"""
    import bench
    rng = np.random.default_rng(seed)
    scale = max(P / 16384.0, 1.0 / 16)
    c = rng.uniform(-0.45 * P, 0.45 * P, K)
    A = rng.uniform(0.2, 3.0, K)
    G = rng.uniform(20.0, 200.0, K) * scale
    rng.uniform(1.0, 20.0, K)
    L = bench.L_FIXED_PIX * scale
    nu_mid = bench.C_LIGHT / (1225.0 * 1e-10)
    sig_hz = G * bench.PIX_HZ / bench.FWHM_PER_SIGMA
    N = A * sig_hz * np.sqrt(2 * np.pi) / bench.SIGMA0
    b = (bench.LINE * 1e-10 * sig_hz * 2.355 / np.sqrt(2)) * 1e-3
    zred = ((bench.C_LIGHT / (nu_mid + bench.PIX_HZ * c)) / 1e-10 - bench.LINE) / bench.LINE
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    return x, np.stack([N, b, zred], axis=1).ravel(), np.array([L, bench.LINE, nu_mid, bench.PIX_HZ])


def headline_case(dtype="f64", data_shift=None, P=16384, K=16):
    x, truth, nbz = headline_truth(P, K)
    return make_case("headline", x, truth, K, mode=vo.MODE_NBZ3, dtype=dtype, nbz=nbz, data_shift=data_shift)


def far_pixel(case):
    """the pixel farthest from every line, in units of the line's width (a far-field pixel of every tile's sweep)"""
    comps = vo.native_components(case.region, case.truth)
    x = case.region.x
    d = np.min([np.abs(x - cm[1]) / max(cm[-1], 1e-300) for cm in comps], axis=0)
    d[:TILE] = d[-TILE:] = 0                          # not in the first or last tile
    return int(np.argmax(d))


def grid(P, kind, rng):
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    if kind == "uneven":
        x = np.cumsum(rng.uniform(0.5, 1.5, P))
        x -= x.mean()
    elif kind == "descending":
        x = x[::-1].copy()
    return x


def line_class_truths(x, rng, wide_max=0.75, far_field_cases=None):
    """{family: (comps [K, 4] (A, c, L, G), pad)} for one grid: the far-field families, widths at the wide-line switch,
    narrow capped lines, y < 1e-9 and y > 4.5, saturated cores, centres on tile borders and +-0.5 px from them, centres
    several tiles off the grid, lines in the ragged last tile.  Line 0 of every family is split (K + 1 lines)."""
    P = x.size
    lo, hi = float(x.min()), float(x.max())
    px = (hi - lo) / (P - 1)
    out = {}

    def draw_c(K):
        return rng.uniform(lo, hi, K)

    for name, (g_lo, g_hi, l_lo, l_hi, a_hi) in (far_field_cases or {}).items():
        K = 12
        t = np.empty((K, 4))
        t[:, 1] = draw_c(K)
        t[:, 3] = rng.uniform(g_lo, g_hi, K) * px
        t[:, 2] = 10.0 ** rng.uniform(l_lo, l_hi, K) * px
        t[:, 0] = rng.uniform(0.3, a_hi, K) if a_hi > 0 else 10.0 ** rng.uniform(0.0, -a_hi, K)
        out["ff " + name] = (t, 0.0)
    edge = 128.0 * 2.0 * np.sqrt(np.log(2.0)) / wide_max * px
    K = 8
    t = np.empty((K, 4))
    t[:, 1] = draw_c(K)
    t[:, 3] = edge * rng.uniform(0.9, 1.1, K)
    t[:, 2] = 10.0 ** rng.uniform(-6, 2.5, K) * px
    t[:, 0] = amp_for_peak(t[:, 2], t[:, 3], rng.uniform(0.05, 3.0, K))
    t[0, 0] = amp_for_peak(t[:1, 2], t[:1, 3], 50.0)[0]
    out["wide switch"] = (t, 0.0)
    K = 10                                          # narrow: capped (one tile spans > 16 units of |z|), G down to 1.5e-3 px
    t = np.empty((K, 4))
    i = rng.integers(0, P, K)
    t[:, 1] = x[i] + rng.uniform(-0.5, 0.5, K) * 10.0 ** rng.uniform(-3, 0, K) * px
    t[:, 3] = 10.0 ** rng.uniform(np.log10(1.5e-3), 1.0, K) * px
    t[:, 2] = 10.0 ** rng.uniform(-4, 0.5, K) * px
    t[:, 0] = amp_for_peak(t[:, 2], t[:, 3], rng.uniform(0.1, 5.0, K))
    out["narrow"] = (t, 0.0)
    K = 8                                           # y = L sqrt(ln 2) / G below 1e-9 (4) and above 4.5 (4)
    t = np.empty((K, 4))
    t[:, 1] = draw_c(K)
    t[:, 3] = 10.0 ** rng.uniform(0.3, 2.0, K) * px
    t[4:, 3] = 10.0 ** rng.uniform(0.3, 1.2, 4) * px
    t[:4, 2] = t[:4, 3] * 10.0 ** rng.uniform(-12, -9.5, 4)
    t[4:, 2] = t[4:, 3] * rng.uniform(6.0, 60.0, 4)
    t[:4, 0] = 500.0                                # the largest amplitude of finite prior: tau ~ 1e-7 .. 1e-9
    t[4:, 0] = amp_for_peak(t[4:, 2], t[4:, 3], rng.uniform(0.2, 3.0, 4))
    out["y extremes"] = (t, 0.0)
    K = 6
    t = np.empty((K, 4))
    t[:, 1] = draw_c(K)
    t[:, 3] = 10.0 ** rng.uniform(0.3, 1.8, K) * px
    t[:, 2] = 10.0 ** rng.uniform(-2, 1, K) * px
    t[:, 0] = amp_for_peak(t[:, 2], t[:, 3], rng.uniform(40.0, 60.0, K))
    out["saturated"] = (t, 0.0)
    borders = np.arange(TILE, P, TILE)
    K = min(12, 3 * borders.size) if borders.size else 3
    t = np.empty((K, 4))
    b = rng.choice(borders, K) if borders.size else np.full(K, P // 2)
    # on the border (half way between pixels b - 1 and b) and on the pixels +-0.5 px from it
    t[:, 1] = [[0.5 * (x[bi - 1] + x[bi]), x[bi], x[bi - 1]][j % 3] for j, bi in enumerate(b)]
    t[:, 3] = 10.0 ** rng.uniform(-0.5, 2.0, K) * px
    t[:, 2] = 10.0 ** rng.uniform(-3, 1.5, K) * px
    t[:, 0] = amp_for_peak(t[:, 2], t[:, 3], rng.uniform(0.2, 3.0, K))
    out["tile borders"] = (t, 0.0)
    K = 6                                           # centres 1 .. 6 tiles beyond either end: broad damped wings
    t = np.empty((K, 4))
    off = np.array([1, 3, 6, 1, 3, 6]) * TILE * px
    t[:, 1] = np.where(np.arange(K) < 3, lo - off, hi + off)
    t[:, 3] = 10.0 ** rng.uniform(1.5, 2.7, K) * px
    t[:, 2] = 10.0 ** rng.uniform(1.0, 2.5, K) * px
    t[:, 0] = amp_for_peak(t[:, 2], t[:, 3], rng.uniform(1.0, 8.0, K))
    out["off grid"] = (t, 7 * TILE * px)
    K = 6                                           # in (and next to) the ragged last tile of the array
    t = np.empty((K, 4))
    last = (P - 1) // TILE * TILE
    j = rng.integers(max(0, last - TILE // 2), P, K)
    t[:, 1] = x[j] + rng.uniform(-0.5, 0.5, K) * px
    t[:, 3] = 10.0 ** rng.uniform(-0.5, 2.0, K) * px
    t[:, 2] = 10.0 ** rng.uniform(-3, 1.0, K) * px
    t[:, 0] = amp_for_peak(t[:, 2], t[:, 3], rng.uniform(0.2, 3.0, K))
    out["ragged tail"] = (t, 0.0)
    return out


def line_class_cases(P, kind, dtype, seed, wide_max=0.75, far_field_cases=None, families=None):
    rng = np.random.default_rng(seed)
    x = grid(P, kind, rng)
    cases = []
    for fam, (t, pad) in line_class_truths(x, rng, wide_max, far_field_cases).items():
        if families is not None and fam not in families:
            continue
        comps, pair = with_split(t, 0, rng.uniform(0.2, 0.8))
        cases.append(make_case("%s P=%d %s" % (fam, P, kind), x, comps.ravel(), comps.shape[0], dtype=dtype, pad=pad,
                               splits=(pair,)))
    return cases


def short_case(name, x, K, rng, dtype, mode=vo.MODE_VOIGT4, sample_sd=False, nbz=None):
    """a short region's truth: lines over the region (start_walkers' ranges), the last two coincident when K >= 2"""
    span = float(x.max() - x.min()) or 1.0
    lo = float(x.min())
    K0 = K - 1 if K >= 2 else K
    t = np.empty((K0, 4))
    t[:, 1] = lo + rng.uniform(0.0, 1.0, K0) * span
    t[:, 2] = rng.uniform(0.02, 0.3, K0) * span
    t[:, 3] = rng.uniform(0.05, 0.5, K0) * span
    if mode == vo.MODE_NBZ3:
        t[:, 2] = nbz[0]
    peak = rng.uniform(0.1, 3.0, K0)
    t[:, 0] = peak if mode == vo.MODE_GAUSS3 else amp_for_peak(t[:, 2], t[:, 3], peak)
    splits = ()
    if K >= 2:
        t, pair = with_split(t, K0 - 1, rng.uniform(0.2, 0.8))
        splits = (pair,)
    return make_case(name, x, native_to_mode(t, mode, nbz), K, mode=mode, dtype=dtype, nbz=nbz, sample_sd=sample_sd,
                     splits=splits)


def native_to_mode(t, mode, nbz=None):
    """[K, 4] (A, c, L, G) in units of x -> theta* of the mode (Gaussian: sigma = G / FWHM_PER_SIGMA, L dropped;
    (N, b, z): through nbz = [l_fixed, line, x_origin, x_scale], L dropped)"""
    t = np.asarray(t, dtype=np.float64)
    if mode == vo.MODE_VOIGT4:
        return t.ravel()
    if mode == vo.MODE_GAUSS3:
        return np.stack([t[:, 0], t[:, 1], t[:, 3] / vo.FWHM_PER_SIGMA], axis=1).ravel()
    _, line, x_origin, x_scale = [float(v) for v in nbz]
    out = [vo.native_to_nbz(a, x_origin + x_scale * c, (g / vo.FWHM_PER_SIGMA) * x_scale, line) for a, c, _, g in t]
    return np.array(out).ravel()
