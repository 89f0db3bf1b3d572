"""GPU tests (-m gpu) of the two kernels that drive the chi^2 sweep, at the shapes and limits the other tests do not reach.

The MAP search (k_map_search, "map_device" = 1, and the host-driven search of csrc/map_search.hpp, "map_device" = 0)
against scipy's fmin (with a stable argsort, _fmin) run region by region on the context's own lnprob, on every launch class (one- and two-line
regions, short regions of 3..8 lines, blends, regions of 9..16 and of 17..32 lines, long regions of the
workgroup-per-walker shape), at the simplex's move from LDS to global scratch (D = 33 / 34) and at D = 129, in every
mode, with and without sd, in both dtypes:
  - fmin's iteration count == the search's + 1, optimum to rtol 1e-13, lnprob_best == -fopt to rtol 1e-13;
  - ctx.lnprob(best) == lnprob_best bit for bit (the search's objective is vamp_lnprob's), and a point's lnprob
    alone == in a batch of other points (no dependence on the walkers that share a wavefront);
  - the optimum scored by the oracle: lnprob to 1e-9 (fp64), chi^2 to 1e-3 (fp32);
  - maxfun: the search checks it at the top of an iteration (PyMC-era fmin), so it equals current fmin run with
    maxiter = its + 1 and no maxfun, whose call count reaches maxfun while the run with maxiter = its stays below.
The map_* functions take a context, so tests/test_cpu_boundary.py runs them through the host ABI as well.

The resident step loop (k_run_resident, "resident" = 2) against one launch per half-step (0) bit for bit and against
the oracle's stretch move, at its limits: regions of 9..16 and 32 lines, W = 254 / 256 (128 movers, the most it
takes) and 258 (falls back), halves that take several rounds of the workgroup's wavefronts, dynamic LDS beyond
48 KB, more than 256 regions.  Which path ran is read from vamp_kernel_timing's count: one timed interval per
vamp_sampler_run on the resident path, one per half-step on the launch path.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import vamp_oracle as vo

pytestmark = pytest.mark.gpu

FPS = 2.0 * np.sqrt(2.0 * np.log(2.0))
C_LIGHT, SIGMA0, LINE, PIX_HZ = 2.98e8, 0.0263, 1215.67, 4.0e10
CK_SHORT, CK_MID, CK_WIDE, CK_SMALL2, CK_XL = 0, 1, 2, 3, 4
NARROW_PX = 1e-3                        # as tests/test_gpu_fp32.py: fp32 cannot resolve lines this narrow

# (pixels, lines) of the spectrum-like MAP contexts: every launch class, 16 and 32 lines, 8 Voigt lines (+ sd: D = 33)
MAP_SHAPES = [(30, 1), (44, 2), (36, 2), (51, 4), (70, 8), (160, 3), (200, 6), (60, 9), (90, 12), (110, 16), (300, 32)]
MAP_LONG_SHAPES = [(2048, 2), (2304, 6), (2100, 9)]        # every region >= 2048 px: one walker per workgroup
# the limits: PyMC's call (MAP.fit(iterlim, tol): fmin's xtol and maxfun at their defaults) and a tight one
LIMITS = {"pymc": dict(iterlim=1000, tol=1e-3), "tight": dict(iterlim=150, tol=1e-9, xtol=1e-9)}
MAP_CASES = ["gauss", "gauss-sd", "voigt", "voigt-sd", "nbz", "long"]


def _expected_kind(P, K, mode):
    if K > 16:
        return CK_XL
    if K > 8:
        return CK_WIDE
    if K <= 2:
        return CK_SMALL2
    return CK_MID if mode != vo.MODE_GAUSS3 and 96 <= P <= 512 else CK_SHORT


def _synthetic(rng, P, K):
    """a region of K absorption lines over P pixels with seeded noise; the lines' (amplitude, centroid, width)"""
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    c = rng.uniform(x[0] * 0.8, x[-1] * 0.8, K)
    w = rng.uniform(1.5, min(0.08 * P + 2.0, 12.0), K)
    tau = sum(rng.uniform(0.3, 2.0) * np.exp(-0.5 * ((x - ck) / wk) ** 2) for ck, wk in zip(c, w))
    return x, np.exp(-tau) + rng.normal(0, 0.02, P), c, w


def _nbz_params(rng, lam_mid=1225.0):
    """(l_fixed, line, x_origin, x_scale) of a region observed around lam_mid Angstrom"""
    return [float(10.0 ** rng.uniform(-1, 0.5)), LINE, C_LIGHT / (lam_mid * 1e-10), PIX_HZ]


def _to_nbz(th, nbz):
    """(amplitude, centroid [px], ., G_fwhm [px]) rows -> (N, b, z) rows of a region with the given nbz parameters"""
    sig_hz = th[:, 3] * PIX_HZ / FPS
    return np.stack([th[:, 0] * sig_hz * np.sqrt(2 * np.pi) / SIGMA0, (LINE * 1e-10 * sig_hz * 2.355 / np.sqrt(2)) * 1e-3,
                     ((C_LIGHT / (nbz[2] + PIX_HZ * th[:, 1])) / 1e-10 - LINE) / LINE], axis=1)


def map_context(case, seed=0):
    """regions, starts near the truth and the set_regions keywords of a MAP test context"""
    mode = {"gauss": vo.MODE_GAUSS3, "nbz": vo.MODE_NBZ3}.get(case.split("-")[0], vo.MODE_VOIGT4)
    sd = case.endswith("-sd")
    shapes = list(MAP_LONG_SHAPES if case == "long" else MAP_SHAPES)
    if case == "gauss-sd":
        shapes.append((90, 11))                          # 11 Gaussians + sd: D = 34, the first simplex in scratch
    rng = np.random.default_rng(900 + 17 * MAP_CASES.index(case) + seed)
    xs, fs, ns, Ks, starts, nbz = [], [], [], [], [], []
    for P, K in shapes:
        x, f, c, w = _synthetic(rng, P, K)
        th = np.empty((K, 4))
        th[:, 0] = rng.uniform(0.3, 1.2, K)
        th[:, 1] = np.clip(c + rng.normal(0, 0.7, K), x[0] * 0.85 + 3, x[-1] * 0.85 - 3)   # 1.05 x centroid: in the prior
        th[:, 2] = rng.uniform(0.2, 2.0, K)
        th[:, 3] = FPS * w * rng.uniform(0.8, 1.25, K)
        if mode == vo.MODE_GAUSS3:
            t = np.stack([th[:, 0], th[:, 1], th[:, 3] / FPS], 1)
        elif mode == vo.MODE_NBZ3:
            nbz.append(_nbz_params(rng, 1216.5))          # z ~ 7e-4: 1.05 z moves a line by ~2 px, not out of the region
            t = _to_nbz(th, nbz[-1])
        else:
            t = th
        xs.append(x); fs.append(f); Ks.append(K)
        ns.append(np.ones(P) if sd else np.full(P, 0.02))
        starts.append(np.concatenate([t.ravel(), [0.04]]) if sd else t.ravel())
    kw = dict(mode=mode, sample_sd=sd)
    if mode == vo.MODE_NBZ3:
        kw["nbz"] = np.array(nbz)
    return xs, fs, ns, Ks, starts, kw


def _oracle_region(x, f, n, K, kw, r):
    reg = vo.Region(x=x, flux=f, noise=n, n_comp=K, mode=kw["mode"], sample_sd=kw.get("sample_sd", False))
    if kw["mode"] == vo.MODE_NBZ3:
        reg.l_fixed, reg.line, reg.x_origin, reg.x_scale = [float(v) for v in kw["nbz"][r]]
    return reg


def _narrow(reg, t, x):
    with np.errstate(all="ignore"):
        comps = vo.native_components(reg, t)
    px = np.median(np.abs(np.diff(x)))
    return any(abs(c[-1] if reg.mode != vo.MODE_GAUSS3 else c[2]) <= NARROW_PX * px for c in comps)


def _objective(ctx, r):
    def neg(t):
        v = ctx.lnprob(t, region=r)[0]
        return -v if np.isfinite(v) else 1e300
    return neg


def _fmin(*args, **kw):
    """scipy's fmin with a stable argsort.  fmin orders its simplex with np.argsort, which is not stable even for a few
    values (numpy's vectorised sorts); the search keeps tied vertices in their order (insertion sort), as the PyMC-era
    fmin did for its simplices of up to 16 vertices.  fp32 objectives tie near an optimum (the fp32 (N, b, z) search
    of a 2-line region: 8 tied sorts in 671 iterations; with numpy's sort fmin's path leaves the search's at the last
    one, with a stable sort it stays on it bit for bit)."""
    import scipy.optimize._optimize as so
    from scipy.optimize import fmin
    real = so.np

    class StableArgsort:
        def __getattr__(self, name):
            return getattr(real, name)

        @staticmethod
        def argsort(a, *a_args, **a_kw):
            return real.argsort(a, kind="stable")

    so.np = StableArgsort()
    try:
        return fmin(*args, **kw)
    finally:
        so.np = real


def _start_simplex(s):
    """fmin's start simplex of s (5 %, 0.00025 for a zero coordinate)"""
    sim = np.tile(s, (s.size + 1, 1))
    for k in range(s.size):
        sim[k + 1, k] = 1.05 * s[k] if s[k] != 0 else 0.00025
    return sim


def _set_map_context(ctx, case):
    xs, fs, ns, Ks, starts, kw = map_context(case)
    ctx.set_regions(xs, fs, ns, Ks, **kw)
    kinds, _ = ctx.region_classes()
    if case == "long":
        assert kinds == [CK_WIDE] * len(xs) and min(len(x) for x in xs) >= 2048
    else:
        assert kinds == [_expected_kind(len(x), K, kw["mode"]) for x, K in zip(xs, Ks)], kinds
        want = {CK_SMALL2, CK_SHORT, CK_WIDE, CK_XL} | ({CK_MID} if kw["mode"] != vo.MODE_GAUSS3 else set())
        assert set(kinds) == want and 16 in Ks and 32 in Ks
    dims = [s.size for s in starts]
    if case == "voigt-sd":
        assert 33 in dims and 129 in dims
    if case == "gauss-sd":
        assert 34 in dims
    # no vertex of a start simplex outside the prior: the start simplex holds no ties at 1e300
    for r, s in enumerate(starts):
        assert np.isfinite(ctx.lnprob(_start_simplex(s), region=r)).all(), (case, r)
    return xs, fs, ns, Ks, starts, kw


def _map_all_capped(ctx, starts, lim, iterlims):
    """vamp_map_all with iterlim per region: one call per distinct limit over the regions that have it (`active`)"""
    best, lnp = [None] * len(starts), np.empty(len(starts))
    chi, its = np.empty(len(starts)), np.zeros(len(starts), dtype=np.int64)
    for it_lim in sorted(set(iterlims)):
        act = np.array([v == it_lim for v in iterlims], dtype=np.uint8)
        b, l, c, i = ctx.map_all(starts, active=act, **dict(lim, iterlim=it_lim))
        for r in np.flatnonzero(act):
            best[r], lnp[r], chi[r], its[r] = b[r], l[r], c[r], i[r]
    return best, lnp, chi, its


def map_follows_fmin(ctx, case, limits, oracle_bar="f64", iter_cap_d129=None):
    """vamp_map_all under `limits` (both map_device settings) against scipy's fmin on -ctx.lnprob region by region;
    iter_cap_d129 caps iterlim of the regions of more than 128 dimensions (a short host run)"""
    xs, fs, ns, Ks, starts, kw = _set_map_context(ctx, case)
    lim = dict(LIMITS[limits])
    iterlims = [min(lim["iterlim"], iter_cap_d129) if iter_cap_d129 and s.size > 128 else lim["iterlim"] for s in starts]
    runs = {}
    try:
        for dev in (1, 0):
            ctx.set_option("map_device", dev)
            runs[dev] = _map_all_capped(ctx, starts, lim, iterlims)
    finally:
        ctx.set_option("map_device", 1)
    (b1, l1, c1, i1), (b0, l0, c0, i0) = runs[1], runs[0]
    assert np.array_equal(i1, i0) and np.array_equal(l1, l0) and np.array_equal(c1, c0, equal_nan=True)
    assert all(np.array_equal(u, v) for u, v in zip(b1, b0))
    skipped = capped = 0
    for r in range(len(xs)):
        tag = (case, limits, r, len(xs[r]), Ks[r])
        # maxfun = 0: 200 evaluations per dimension, the default of the PyMC-era fmin (current scipy sets no cap once
        # maxiter is given, so the cap is passed explicitly)
        cap = lim.get("maxfun") or 200 * starts[r].size
        xopt, fopt, it, calls, _ = _fmin(_objective(ctx, r), starts[r], xtol=lim.get("xtol", 1e-4), ftol=lim["tol"],
                                        maxiter=iterlims[r], maxfun=cap, disp=False, full_output=True)
        if calls >= cap:        # maxfun ended the search: the PyMC-era rule, pinned by map_maxfun_rule
            capped += 1
            xopt, fopt, it = _fmin_at_top_of_loop(ctx, r, starts[r], lim.get("xtol", 1e-4), lim["tol"], int(i1[r]), cap, tag)
        assert it == i1[r] + 1, tag + (it, i1[r])              # fmin counts iterations from 1
        assert np.allclose(b1[r], xopt, rtol=1e-13, atol=0), tag
        assert np.isclose(l1[r], -fopt, rtol=1e-13, atol=0), tag + (l1[r], -fopt)
        lb, cb = ctx.lnprob(b1[r], region=r, return_chi2=True)
        assert lb[0] == l1[r] and (cb[0] == c1[r] or (np.isnan(cb[0]) and np.isnan(c1[r]))), tag
        assert l1[r] >= ctx.lnprob(starts[r], region=r)[0]
        reg = _oracle_region(xs[r], fs[r], ns[r], Ks[r], kw, r)
        want, wchi = vo.log_prob_batch(reg, b1[r][None, :], return_chi2=True)
        assert np.isfinite(want[0]), tag
        if oracle_bar == "f64":
            assert abs(l1[r] - want[0]) <= 1e-9 * max(1.0, abs(want[0])), tag + (l1[r], want[0])
        elif _narrow(reg, b1[r], xs[r]):
            skipped += 1
        else:
            assert abs(c1[r] - wchi[0]) <= 1e-3 * wchi[0], tag + (c1[r], wchi[0])
            assert abs(l1[r] - want[0]) <= 1e-3 * max(1.0, abs(want[0])), tag + (l1[r], want[0])
    assert skipped <= len(xs) // 3, (case, limits, skipped)           # fp32: optima with a line narrower than 1e-3 px
    if limits == "tight":
        assert (i1 + 1 == np.array(iterlims)).sum() >= len(xs) // 2, i1      # maxiter is what stops most searches
    return i1, capped


def _fmin_at_top_of_loop(ctx, r, start, xtol, ftol, its, maxfun, tag):
    """fmin with maxfun checked at the top of the loop only (the PyMC-era rule) for a search of `its` updates that
    maxfun ended: current fmin run for its + 1 iterations without a cap reaches maxfun, run for its it does not"""
    neg = _objective(ctx, r)
    xopt, fopt, it, calls, _ = _fmin(neg, start, xtol=xtol, ftol=ftol, maxiter=its + 1, maxfun=10 ** 9, disp=False,
                                    full_output=True)
    assert calls >= maxfun, tag + (it, calls)
    calls_before = _fmin(neg, start, xtol=xtol, ftol=ftol, maxiter=its, maxfun=10 ** 9, disp=False, full_output=True)[3]
    assert calls_before < maxfun, tag + (calls_before,)
    return xopt, fopt, it


MAXFUN = 200
# regions per context whose search maxfun stops inside an iteration (fmin's count at its + 1 above MAXFUN): 3, 1 and 5
MID_ITERATION_MIN = {"gauss-sd": 2, "voigt-sd": 1, "nbz": 3}


def map_maxfun_rule(ctx, case, maxfun=MAXFUN):
    """maxfun stops the search at the top of an iteration (the PyMC-era fmin rule; current scipy stops inside the
    iteration at the call that would exceed it): the search equals fmin with maxiter = its + 1 and no maxfun,
    whose call count reaches maxfun, and the same run with maxiter = its stays below maxfun.  Returns, per region,
    (its, fmin's calls at its + 1 iterations, current scipy's iteration count under maxfun)."""
    xs, fs, ns, Ks, starts, kw = _set_map_context(ctx, case)
    lim = dict(iterlim=10 ** 6, tol=0.0, xtol=0.0, maxfun=maxfun)            # no stopping test: maxfun decides
    runs = {}
    try:
        for dev in (1, 0):
            ctx.set_option("map_device", dev)
            runs[dev] = ctx.map_all(starts, **lim)
    finally:
        ctx.set_option("map_device", 1)
    (b1, l1, _, i1), (b0, l0, _, i0) = runs[1], runs[0]
    assert np.array_equal(i1, i0) and np.array_equal(l1, l0) and all(np.array_equal(u, v) for u, v in zip(b1, b0))
    out = []
    for r in range(len(xs)):
        neg = _objective(ctx, r)
        tag = (case, r, Ks[r], int(i1[r]))
        xopt, fopt, it = _fmin_at_top_of_loop(ctx, r, starts[r], 0.0, 0.0, int(i1[r]), maxfun, tag)
        assert it == i1[r] + 1, tag + (it,)
        assert np.allclose(b1[r], xopt, rtol=1e-13, atol=0) and np.isclose(l1[r], -fopt, rtol=1e-13, atol=0), tag
        calls = _fmin(neg, starts[r], xtol=0.0, ftol=0.0, maxiter=it, maxfun=10 ** 9, disp=False, full_output=True)[3]
        _, _, it_now, calls_now, _ = _fmin(neg, starts[r], xtol=0.0, ftol=0.0, maxiter=10 ** 6, maxfun=maxfun,
                                          disp=False, full_output=True)
        assert calls_now == maxfun and it_now <= it, tag + (it_now, calls_now)
        out.append((int(i1[r]), int(calls), int(it_now)))
    # maxfun runs out INSIDE an iteration for several regions: there the PyMC-era rule finishes it, current fmin not
    assert sum(c > maxfun for _, c, _ in out) >= MID_ITERATION_MIN.get(case, 1), out
    return out


@pytest.mark.parametrize("limits", list(LIMITS))
@pytest.mark.parametrize("case", MAP_CASES)
def test_map_search_follows_fmin_on_every_class(case, limits):
    import vamp_amd
    with vamp_amd.HipContext(device=0) as ctx:
        its, capped = map_follows_fmin(ctx, case, limits)
    print(case, limits, "iterations", its.tolist(), "ended by maxfun:", capped)


def point_alone_equals_point_in_a_batch(ctx, case, n=64):
    """vamp_lnprob of each of n points alone == the same point among n spread-out points, bit for bit, in every region
    of a MAP context.  A walker's value must not depend on the walkers that share its wavefront (packed shapes): the
    MAP search evaluates its candidates in batches and promises the bits vamp_lnprob gives a single point."""
    xs, fs, ns, Ks, starts, kw = _set_map_context(ctx, case)
    rng = np.random.default_rng(77 + MAP_CASES.index(case))
    for r, s in enumerate(starts):
        pts = s * rng.uniform(0.6, 1.4, (n, s.size))            # lines near and far from each other's pixels
        batch = ctx.lnprob(pts, region=r)
        alone = np.array([ctx.lnprob(p, region=r)[0] for p in pts])
        assert np.isfinite(alone).sum() >= n // 4, (case, r)
        assert np.array_equal(batch, alone), (case, r, int((batch != alone).sum()))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", MAP_CASES)
def test_point_alone_equals_point_in_a_batch(case, dtype):
    import vamp_amd
    with vamp_amd.HipContext(device=0, dtype=vamp_amd.F64 if dtype == "f64" else vamp_amd.F32) as ctx:
        point_alone_equals_point_in_a_batch(ctx, case)


@pytest.mark.parametrize("case", ["gauss-sd", "voigt-sd", "nbz"])
def test_map_search_maxfun_rule(case):
    import vamp_amd
    with vamp_amd.HipContext(device=0) as ctx:
        out = map_maxfun_rule(ctx, case)
    print(case, "(its, fmin calls at its + 1, current fmin iterations)", out)


@pytest.mark.parametrize("limits", list(LIMITS))
@pytest.mark.parametrize("case", MAP_CASES)
def test_fp32_map_search_follows_fmin_on_every_class(case, limits):
    import vamp_amd
    with vamp_amd.HipContext(device=0, dtype=vamp_amd.F32) as ctx:
        map_follows_fmin(ctx, case, limits, oracle_bar="f32")


# ---- the resident step loop at its limits --------------------------------------------------------------------------
def _walkers(rng, shapes, W, variant):
    """regions of the given (pixels, lines) and W start walkers each; variant 0: Voigt, 1: Gaussian, 2: Voigt + sd,
    3: (N, b, z)"""
    xs, fs, ns, Ks, ths, nbz = [], [], [], [], [], []
    for P, K in shapes:
        x, f, c, w = _synthetic(rng, P, K)
        th = np.empty((W, K, 4))
        th[:, :, 0] = rng.uniform(0.2, 1.5, (W, K))
        th[:, :, 1] = c + rng.normal(0, 1.5, (W, K))
        th[:, :, 2] = 10.0 ** rng.uniform(-2, 0.5, (W, K))
        th[:, :, 3] = FPS * w * rng.uniform(0.6, 1.6, (W, K))
        th[: max(1, W // 8), 0, 0] = -0.1                       # a few walkers start outside the prior
        xs.append(x); fs.append(f); Ks.append(K)
        ns.append(np.ones(P) if variant == 2 else np.full(P, 0.02))
        if variant == 1:
            t = np.stack([th[:, :, 0], th[:, :, 1], th[:, :, 3] / FPS], axis=2).reshape(W, 3 * K)
        elif variant == 2:
            t = np.hstack([th.reshape(W, 4 * K), rng.uniform(0.01, 0.2, (W, 1))])
        elif variant == 3:
            nbz.append(_nbz_params(rng))
            t = _to_nbz(th.reshape(W * K, 4), nbz[-1]).reshape(W, 3 * K)
        else:
            t = th.reshape(W, 4 * K)
        ths.append(np.ascontiguousarray(t))
    kw = [dict(mode=vo.MODE_VOIGT4), dict(mode=vo.MODE_GAUSS3), dict(mode=vo.MODE_VOIGT4, sample_sd=True), dict(mode=vo.MODE_NBZ3)][variant]
    if variant == 3:
        kw["nbz"] = np.array(nbz)
    return xs, fs, ns, Ks, ths, kw


def resident_plan(ctx):
    """(kind, compute wavefronts, walkers per round, dynamic LDS bytes) of every resident workgroup (test hook)"""
    fn = ctx._lib.vampdbg_resident_plan
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    n = fn(ctx._h, 0, (C.c_longlong * 4)())
    assert n >= 1
    rows = (C.c_longlong * (4 * n))()
    assert fn(ctx._h, n, rows) == n
    return [tuple(rows[4 * i:4 * i + 4]) for i in range(n)]


SHAPES_WIDE = [(30, 1), (44, 2), (51, 4), (160, 3), (60, 9), (90, 12), (110, 16), (300, 32)]
RESIDENT_CASES = {       # shapes, W, variant, path of resident = 2 ("resident" / "launch"), classes that must be present
    "wide-xl": (SHAPES_WIDE, 32, 0, "resident", {CK_SHORT, CK_MID, CK_WIDE, CK_XL}),
    "w256": (SHAPES_WIDE, 256, 2, "resident", {CK_SHORT, CK_MID, CK_WIDE, CK_XL}),
    "w254": ([(44, 2), (70, 6), (60, 9), (120, 16)], 254, 1, "resident", {CK_SHORT, CK_WIDE}),
    "w258": ([(44, 2), (160, 5), (60, 12), (300, 32)], 258, 3, "launch", {CK_SMALL2, CK_MID, CK_WIDE, CK_XL}),
    "regions300": ([(20 + i % 40, 1 + i % 2) for i in range(300)], 32, 0, "resident", {CK_SMALL2}),
}


def _run_three(ctx, ths, W, block):
    ctx.sampler_init(ths, seed=4242, split_block=block)
    ctx.kernel_timing(True)
    a = ctx.run_flat(7, thin=3)
    b = ctx.run_flat(4, thin=1)
    ctx.run(3, store_chain=False)
    _, launches = ctx.kernel_timing(False)
    return a, b, ctx.get_state(), launches


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", list(RESIDENT_CASES))
def test_resident_loop_at_its_limits(case, dtype):
    import vamp_amd
    shapes, W, variant, path, kinds_want = RESIDENT_CASES[case]
    rng = np.random.default_rng(5100 + list(RESIDENT_CASES).index(case))
    xs, fs, ns, Ks, ths, kw = _walkers(rng, shapes, W, variant)
    block = 2 if W % 4 else 8
    dt = vamp_amd.F64 if dtype == "f64" else vamp_amd.F32
    out = {}
    with vamp_amd.HipContext(device=0, dtype=dt) as ctx:
        ctx.set_regions(xs, fs, ns, Ks, **kw)
        kinds, _ = ctx.region_classes()
        assert set(kinds) >= kinds_want, kinds
        for resident in (2, 0):
            ctx.set_option("resident", resident)
            out[resident] = _run_three(ctx, ths, W, block)
        if case == "regions300":
            # the automatic policy leaves more than 256 regions on the launch path: a resident workgroup each would queue
            ctx.set_option("resident", 1)
            out[1] = _run_three(ctx, ths, W, block)
            ctx.set_option("resident", 2)
        plan = resident_plan(ctx) if path == "resident" else None
        ctx.set_option("resident", 1)
        ev = None
        if dtype == "f32":
            ev = vamp_amd.HipContext(device=0, dtype=vamp_amd.F32)
            ev.set_regions(xs, fs, ns, Ks, **kw)
    try:
        (a2, b2, s2, n2), (a0, b0, s0, n0) = out[2], out[0]
        assert n0 == 2 * 14, n0                                   # launch path: a timed launch per half-step
        assert n2 == (3 if path == "resident" else 2 * 14), (case, n2)
        if case == "regions300":
            assert out[1][3] == 2 * 14
            assert all(np.array_equal(u, v) for u, v in zip(out[1][0][:3], a0[:3]))
        if plan is not None:
            print(case, dtype, "W", W, "resident workgroups (kind, nw, walkers per round, LDS bytes):", plan)
            assert all(nw >= 1 for _, nw, _, _ in plan)
            if case == "w256":
                assert any(per_round < W // 2 for _, _, per_round, _ in plan)          # a half-step takes several rounds
                assert any(lds > 48 * 1024 for _, _, _, lds in plan)                   # hipFuncSetAttribute path
        for x2, x0 in ((a2, a0), (b2, b0)):
            assert x2[0].shape == x0[0].shape and x2[0].shape[0] in (2, 4)
            assert np.array_equal(x2[0], x0[0]) and np.array_equal(x2[1], x0[1]) and np.array_equal(x2[2], x0[2])
        assert s2[3] == s0[3] == 14
        for r in range(len(xs)):
            assert np.array_equal(s2[0][r], s0[0][r]) and np.array_equal(s2[1][r], s0[1][r]) and np.array_equal(s2[2][r], s0[2][r]), r
        assert a2[2].sum() > 0
        # the resident chain replayed by the oracle's stretch move (11 steps: the two stored runs)
        offs = np.concatenate([[0], np.cumsum([W * t.shape[1] for t in ths])])
        check = range(len(xs)) if len(xs) <= 16 else range(0, len(xs), 23)
        for r in check:
            D = ths[r].shape[1]
            if ev is None:
                reg = _oracle_region(xs[r], fs[r], ns[r], Ks[r], kw, r)
                fn = lambda q, reg=reg: vo.log_prob_batch_fast(reg, q)
            else:
                fn = lambda q, r=r: ev.lnprob(np.concatenate([q, q]), region=r)[:len(q)]
            lnp0 = fn(ths[r]) if ev is None else ev.lnprob(ths[r], region=r)        # W points: the shape of sampler_init
            chain, lchain, nacc = vo.run_sampler_batch(fn, ths[r], lnp0, 11, seed=4242, block=block, region=r,
                                                       walker_off=r * W)
            got = np.concatenate([a2[0], b2[0]])[:, offs[r]:offs[r + 1]].reshape(-1, W, D)
            want = chain[[2, 5, 7, 8, 9, 10]]
            assert np.allclose(got, want, rtol=1e-10, atol=1e-12), (case, dtype, r)
            glp = np.concatenate([a2[1], b2[1]])[:, r * W:(r + 1) * W]
            assert np.allclose(glp, lchain[[2, 5, 7, 8, 9, 10]], rtol=1e-9, atol=1e-9), (case, dtype, r)
            assert np.array_equal(b2[2][r * W:(r + 1) * W], nacc), (case, dtype, r)
    finally:
        if ev is not None:
            ev.close()
