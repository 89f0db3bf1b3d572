"""The far-field sweep reads a tile's geometry -- (mid, half) per full tile, the pixels' places in their quarters --
from tables that vamp_set_regions builds once per context (k_tile_tables), and takes the guards of the node evaluation
(ff_eval2: the clamp at X_FAR and its patch, the e^{-x^2} patch for y < Y_TINY) only for walkers whose lines can need
them: two bits per walker, decided at staging (ff_guard_bits).  Both leave every computed value what it was, so
"equal" below means bit-equal; against the oracle the bars are those of tests/test_gpu_parity.py: fp64
|delta lnprob| <= 1e-9 max(1, |lnprob|), fp32 1e-3 relative, sampler positions to 1e-10 with identical accept counts.

What can go wrong and where it is looked for:
  - the tables are indexed by GLOBAL pixel (u) and by global pixel >> 8 (geometry) while tiles start at multiples of 256
    pixels of their REGION: three regions whose offsets (0, 300, 2704) are no multiple of 256, each against itself alone;
  - a context that is given new regions must not read the tables of the old ones: three set_regions calls on one context;
  - the orientation of the grid travels in the sign of the stored half-width, the quarter of a pixel depends on it:
    ascending, descending and alternating-spacing grids, fp64 and fp32, lnprob and two sampler steps;
  - a guard bit of one walker must not reach another walker of the launch, and a walker that needs a guard must get it:
    planted walkers among ordinary ones, every walker against itself evaluated alone.
The CPU half restates the two predicates in numpy and asserts that the planted walkers set them and the ordinary ones do
not (else nothing here would run the unguarded loop), and that the oracle is finite for every walker of every case."""
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo

TILE = 256
W = 64
SD = 0.05
Y_TINY, X_FAR = 1.0e-9, 1.0e4          # voigt_math.hpp
KS = (1, 7, 16)
PACKINGS = (256, 64)                   # workgroup per walker (Taylor tables) / wavefront per walker: forced, so that a region
                                       # runs one kernel shape whatever else its context holds
INDEX_REGIONS = ((300, "up"), (2404, "up"), (2304, "up"))           # pix_off 0, 300, 2704
STALE_REGIONS = ((4352, "steps"), (2304, "down"), (300, "up"))
GRIDS = tuple((P, kind) for kind in ("up", "down", "steps") for P in (2304, 4352))


def make_grid(P, kind):
    if kind == "steps":                # tiles of unit and of double pixel spacing alternate
        x = np.cumsum(np.where((np.arange(P) // TILE) % 2 == 0, 1.0, 2.0))
        return x - 0.5 * (x[0] + x[-1])
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    return x[::-1].copy() if kind == "down" else x


def make_lines(x, K, rng):
    """[K, 4] rows (A, c, L, G): damped wings, narrow lines on tile borders, lines whose far tiles need the deep
    fractions, lines whose |z| < 8 zone reaches two half-widths away, lines wider than a tile -- every class of
    ff_classify_batch, with centroids on tile borders and just outside the region."""
    xa = np.sort(x)
    P, dx, span = xa.size, np.max(np.diff(xa)), xa[-1] - xa[0]
    inside = lambda lo, hi: xa[0] + rng.uniform(lo, hi) * span
    border = lambda i: 0.5 * (xa[TILE * i - 1] + xa[TILE * i]) if 0 < TILE * i < P else inside(0.3, 0.7)
    past = lambda d: min(border(1) + d * dx, xa[-1] + 20.0 * dx)      # d pixels past the first border, inside the prior
    last = max(P // TILE - 1, 1)
    kinds = {
        "damped": lambda c: (10.0 ** rng.uniform(0.5, 2.4), c, rng.uniform(30, 300), rng.uniform(5, 30)),
        "narrow": lambda c: (rng.uniform(0.5, 5.0), c, 10.0 ** rng.uniform(-2, 0), rng.uniform(2, 18)),
        "medium": lambda c: (rng.uniform(0.5, 3.0), c, 10.0 ** rng.uniform(-1, 0.5), rng.uniform(40, 60) * dx),
        "broad": lambda c: (rng.uniform(0.3, 1.5), c, 10.0 ** rng.uniform(-1, 0.5), rng.uniform(175, 190) * dx),
        "wide": lambda c: (rng.uniform(10.0, 30.0), c, rng.uniform(5.0, 15.0), rng.uniform(310, 400) * dx),
    }
    if K == 1:
        plan = [("medium", past(100.0))]
    elif K == 7:
        plan = [("damped", xa[-1] + 5.0 * dx), ("narrow", border(1)), ("medium", past(150.0)), ("broad", inside(0.1, 0.4)),
                ("wide", inside(0.0, 1.0)), ("narrow", inside(0.5, 0.9)), ("damped", border(last))]
    else:
        plan = [("damped", xa[0] - 3.0 * dx), ("damped", xa[-1] + 5.0 * dx), ("damped", past(160.0)),
                ("narrow", border(1)), ("narrow", border(2)), ("narrow", inside(0.05, 0.3)), ("narrow", inside(0.6, 1.0)),
                ("narrow", border(last)), ("medium", past(180.0)), ("medium", inside(0.1, 0.3)), ("medium", inside(0.5, 1.0)),
                ("broad", inside(0.0, 0.3)), ("broad", inside(0.4, 0.7)), ("broad", inside(0.7, 1.0)),
                ("wide", inside(0.0, 1.0)), ("wide", inside(0.0, 1.0))]
    assert len(plan) == K
    t = np.array([kinds[kind](c) for kind, c in plan])
    return t[rng.permutation(K)]


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _region(x, t, K, rng):
    noise = np.full(x.size, SD)
    pad = 50.0 * np.max(np.abs(np.diff(x)))
    bounds = np.array([[x.min() - pad, x.max() + pad, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=vo.MODE_VOIGT4, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    flux = vo.model_flux(vo.Region(x=x, flux=np.ones(x.size), noise=noise, **kw), t.reshape(-1)) + rng.normal(0, SD, x.size)
    return noise, bounds, flux, vo.Region(x=x, flux=flux, noise=noise, **kw)


@functools.lru_cache(maxsize=None)
def case(P, kind, K):
    """Grid, data, W walkers (the same lines rotated, walker 0 exact, the others moved by 1e-4) and the oracle's
    log-posteriors of one (grid, K): computed once, shared, read-only."""
    x = make_grid(P, kind)
    rng = np.random.default_rng(100 * P + 10 * K + len(kind))
    t = make_lines(x, K, rng)
    noise, bounds, flux, reg = _region(x, t, K, rng)
    th = np.empty((W, 4 * K))
    for w in range(W):
        tw = t * (1.0 + (1e-4 if w else 0.0) * rng.standard_normal(t.shape))
        th[w] = np.roll(tw, w % K, axis=0).reshape(-1)
    return _freeze(dict(x=x, flux=flux, noise=noise, th=th, want=vo.log_prob_batch_fast(reg, th), bounds=bounds, reg=reg, K=K))


# ---- the guards ------------------------------------------------------------------------------------------------------
GUARD_P, GUARD_K = 2304, 7
PLANTED = {5: ("tiny",), 22: ("reach",), 41: ("tiny", "reach")}      # walker: the lines planted in it ...
SLOT = {"tiny": 1, "reach": 4}                                       # ... in place of its lines 1 / 4


@functools.lru_cache(maxsize=None)
def guard_case():
    c = case(GUARD_P, "up", GUARD_K)
    x = c["x"]
    th = c["th"].copy().reshape(W, GUARD_K, 4)
    hub = 0.5 * (x[TILE] + x[2 * TILE - 1])          # middle of the second tile
    special = {
        # y = 8e-11; |z| = 8 lies 4.8 G = 384 px from the centre: inside the tiles two and more away, which are far
        "tiny": (1.5, hub, 80.0 * 1.0e-10, 80.0),
        # s = 33 per pixel: the region's far end is at X = 5e4 > X_FAR
        "reach": (2.0, hub + 40.3, 0.01, 0.05),
    }
    for w, names in PLANTED.items():
        for name in names:
            th[w, SLOT[name]] = special[name]
    th = th.reshape(W, -1)
    return _freeze(dict(c, th=th, want=vo.log_prob_batch_fast(c["reg"], th)))


def guard_bits(x, th, K):
    """ff_guard_bits in numpy: per walker, (some line has y < Y_TINY, some line can reach X > X_FAR inside the region)."""
    t = th.reshape(th.shape[0], K, 4)
    c, L, G = t[:, :, 1], t[:, :, 2], t[:, :, 3]
    s, y = 2.0 * vo.SQRT_LN2 / G, L * vo.SQRT_LN2 / G
    reach = s * np.maximum(np.abs(x[0] - c), np.abs(x[-1] - c))
    return (y < Y_TINY).any(1), (reach > X_FAR).any(1)


def test_planted_walkers_set_the_guard_bits_and_no_other_does():
    g = guard_case()
    tiny, reach = guard_bits(g["x"], g["th"], GUARD_K)
    for w in range(W):
        names = PLANTED.get(w, ())
        assert tiny[w] == ("tiny" in names) and reach[w] == ("reach" in names), (w, names, tiny[w], reach[w])
    assert np.isfinite(g["want"]).all()
    # the |z| = 8 border of the tiny-y line falls into far tiles: some tile is >= 2 half-widths and >= w8 away, and closer than w8 + a tile
    x, (A, c, L, G) = g["x"], g["th"][5].reshape(GUARD_K, 4)[SLOT["tiny"]]
    lo, hi = x[::TILE][:GUARD_P // TILE], x[TILE - 1::TILE]
    dist = np.abs(0.5 * (lo + hi) - c) - 0.5 * np.abs(hi - lo)
    w8 = 8.0 * G / (2.0 * vo.SQRT_LN2)
    assert ((dist >= np.abs(hi - lo)) & (dist >= w8) & (dist < w8 + TILE)).any()


ALL_CASES = sorted({(P, kind, K) for P, kind in INDEX_REGIONS for K in KS} | {(P, kind, 7) for P, kind in STALE_REGIONS} |
                   {(P, kind, K) for P, kind in GRIDS for K in (7, 16)})


@pytest.mark.parametrize("P,kind,K", ALL_CASES)
def test_oracle_is_finite_and_no_ordinary_walker_sets_a_guard_bit(P, kind, K):
    c = case(P, kind, K)
    assert np.isfinite(c["want"]).all()
    tiny, reach = guard_bits(c["x"], c["th"], K)
    assert not tiny.any() and not reach.any()


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _ctx(dtype, packing):
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0, dtype=vamp_amd.F64 if dtype == "f64" else vamp_amd.F32)
    ctx.set_packing(packing)
    return ctx


def _set(ctx, cases):
    import vamp_amd
    ctx.set_regions([c["x"] for c in cases], [c["flux"] for c in cases], [c["noise"] for c in cases], [c["K"] for c in cases],
                    mode=vamp_amd.MODE_VOIGT4, bounds=np.vstack([c["bounds"] for c in cases]))


def _check_oracle(dtype, got, want, what):
    assert np.isfinite(want).all() and np.isfinite(got).all(), what
    if dtype == "f64":
        err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
        print(f"{what}: |lnprob| ~ {np.abs(want).mean():.3e}, worst error {err:.2e} (bar 1e-9)")
        assert err <= 1e-9, what
    else:
        err = np.max(np.abs(got - want) / np.abs(want))
        print(f"{what}: |lnprob| ~ {np.abs(want).mean():.3e}, worst error {err:.2e} (bar 1e-3)")
        assert err <= 1e-3, what


def _alone(dtype, packing, c):
    with _ctx(dtype, packing) as ctx:
        _set(ctx, [c])
        return ctx.lnprob(c["th"])


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("packing", PACKINGS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_table_indexing_across_regions(dtype, packing, K):
    cases = [case(P, kind, K) for P, kind in INDEX_REGIONS]
    with _ctx(dtype, packing) as ctx:
        _set(ctx, cases)
        together = [ctx.lnprob(c["th"], region=r) for r, c in enumerate(cases)]
    for r, c in enumerate(cases):
        what = f"{dtype} pack {packing} K={K} region {r} (P={c['x'].size})"
        assert np.array_equal(together[r], _alone(dtype, packing, c)), what
        _check_oracle(dtype, together[r], c["want"], what)


@pytest.mark.gpu
@pytest.mark.parametrize("packing", PACKINGS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_stale_tables(dtype, packing):
    cases = [case(P, kind, 7) for P, kind in STALE_REGIONS]
    with _ctx(dtype, packing) as ctx:
        for c in cases:
            _set(ctx, [c])
            got = ctx.lnprob(c["th"])
            what = f"{dtype} pack {packing} after set_regions(P={c['x'].size})"
            assert np.array_equal(got, _alone(dtype, packing, c)), what
            _check_oracle(dtype, got, c["want"], what)


@pytest.mark.gpu
@pytest.mark.parametrize("P,kind", GRIDS)
@pytest.mark.parametrize("packing", PACKINGS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_grids_match_oracle(dtype, packing, P, kind):
    c = case(P, kind, 16)
    _check_oracle(dtype, _alone(dtype, packing, c), c["want"], f"{dtype} pack {packing} P={P} {kind} K=16")


@pytest.mark.gpu
@pytest.mark.parametrize("P,kind", GRIDS)
@pytest.mark.parametrize("packing", PACKINGS)
def test_two_sampler_steps_match_oracle(packing, P, kind):
    c = case(P, kind, 7)
    with _ctx("f64", packing) as ctx:
        _set(ctx, [c])
        ctx.sampler_init(c["th"], seed=P, a=2.0, split_block=W)
        res = ctx.run(2)
    chain, lchain, nacc = vo.run_sampler(lambda q: vo.log_prob_batch_fast(c["reg"], q), c["th"], c["want"], 2, seed=P, block=W)
    assert np.array_equal(res["n_accept"], nacc)
    assert np.allclose(res["chain"], chain, rtol=1e-10, atol=1e-12)
    assert np.allclose(res["lnprob"], lchain, rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("packing", PACKINGS)
def test_guard_bits_stay_with_their_walker(packing):
    g = guard_case()
    with _ctx("f64", packing) as ctx:
        _set(ctx, [g])
        batch = ctx.lnprob(g["th"])
        alone = np.array([ctx.lnprob(g["th"][w:w + 1])[0] for w in range(W)])
    differ = np.flatnonzero(batch != alone)
    assert differ.size == 0, (packing, differ, batch[differ], alone[differ])
    _check_oracle("f64", batch, g["want"], f"f64 pack {packing} guards")
