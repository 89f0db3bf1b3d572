"""The far-field sweep classifies the lines of a walker against four of a wavefront's tiles in one 64-lane pass
(ff_classify_batch) and leaves the four tiles' far and wide lists in LDS.  These tests run the sweep where batching
can go wrong -- partial batches, wavefronts of one workgroup that disagree on the batch length, a batch plus one tile,
a ragged tail, a descending and a non-uniform grid -- on lines placed so that a dropped, duplicated or misplaced list
entry moves the log-posterior far beyond the bar: strong damped wings (amplitudes up to 300, L of 30 - 300 px), lines
narrower than 20 px, lines wider than a tile (G_fwhm > 300 px, in units of the widest pixel), centroids on tile borders
and just outside the region's ends.  Every walker holds the same lines in a different (rotated) order, so the lists'
compaction sees 16 arrangements of the masks.

Bars: those of tests/test_gpu_parity.py -- fp64 |delta lnprob| <= 1e-9 max(1, |lnprob|), fp32 1e-3 relative; the
sampler's positions to 1e-10 with identical accept counts.

The conditions the shapes are chosen for are asserted on the CPU (test_shapes_cover_every_class) by a few lines of
numpy that restate the kernel's predicates: with K = 16 every shape has (line, tile) pairs that are far-deep,
far-shallow, mid, wide and near, and tiles with at most 8 and with more than 8 far lines (in the fp64 and in the fp32
sense of "far"); with K = 7 all five classes occur (7 lines cannot give a tile more than 8 far ones); one line alone
is far from some tiles and near to others.  Every walker's log-posterior is finite in every case."""
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo

TILE = 256
W = 64
SD = 0.05
FF_DIST, MID_Z2, WIDE_MAX = 2.0, 30.25, 0.75      # VAMP_FF_DIST, VAMP_MID_Z2, VAMP_WIDE_MAX of vamp_hip.hip
SHAPES = {            # name: (pixels, grid)        tiles per wavefront of the 4-wavefront workgroup
    "P2048": (2048, "up"),         # 2 each: one partial batch
    "P2304": (2304, "up"),         # 3 / 2 / 2 / 2: the wavefronts disagree on the batch length
    "P4352": (4352, "up"),         # 5 / 4 / 4 / 4
    "P5120": (5120, "up"),         # 5 each: a full batch plus one
    "P8448": (8448, "up"),         # 9 / 8 / 8 / 8: two full batches plus one
    "P2404": (2404, "up"),         # full tiles plus a tail of 100 px
    "P2304-down": (2304, "down"),
    "P4352-steps": (4352, "steps"),    # tiles of unit and of double pixel spacing alternate
}
KS = (1, 7, 16)


def grid(name):
    P, kind = SHAPES[name]
    if kind == "steps":
        dx = np.where((np.arange(P) // TILE) % 2 == 0, 1.0, 2.0)
        x = np.cumsum(dx)
        return x - 0.5 * (x[0] + x[-1])
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    return x[::-1].copy() if kind == "down" else x


def lines(name, K):
    """[K, 4] rows (A, c, L, G) in units of x.  Line kinds: damped (strong Lorentzian wings), narrow (< 20 px), medium
    (far tiles need the deep fractions), broad (|z| < 8 reaches tiles 2 half-widths away: "mid"), wide (smooth over every
    tile).  A cluster in the second tile keeps that tile's far list short; the other tiles' lists are long."""
    x = grid(name)
    P = x.size
    rng = np.random.default_rng(1000 * P + K)
    xa = np.sort(x)
    dxmax = np.max(np.diff(xa))
    edge = lambda i: 0.5 * (xa[TILE * i - 1] + xa[TILE * i])          # border between tiles i - 1 and i (ascending order)
    ntile = P // TILE
    hub = 0.5 * (xa[TILE] + xa[2 * TILE - 1])                         # middle of the second tile
    kinds = {
        "damped": lambda c: (10.0 ** rng.uniform(0.5, 2.477), c, rng.uniform(30, 300), rng.uniform(5, 30)),
        "narrow": lambda c: (rng.uniform(0.5, 5.0), c, 10.0 ** rng.uniform(-2, 0), rng.uniform(2, 18)),
        "medium": lambda c: (rng.uniform(0.5, 3.0), c, 10.0 ** rng.uniform(-1, 0.5), rng.uniform(40, 60) * dxmax),
        "broad": lambda c: (rng.uniform(0.3, 1.5), c, 10.0 ** rng.uniform(-1, 0.5), rng.uniform(175, 190) * dxmax),
        "wide": lambda c: (rng.uniform(10.0, 30.0), c, rng.uniform(5.0, 15.0), rng.uniform(310, 400) * dxmax),
    }
    if K == 1:
        plan = [("medium", hub)]
    elif K == 7:
        plan = [("damped", xa[-1] + 5.0 * dxmax), ("narrow", edge(1)), ("medium", hub + 40.0), ("broad", hub - 60.0),
                ("wide", rng.uniform(xa[0], xa[-1])), ("narrow", hub + 90.0), ("damped", edge(ntile - 1))]
    else:
        far_end = lambda: rng.uniform(xa[3 * TILE], xa[-1])
        plan = [("damped", xa[0] - 3.0 * dxmax), ("damped", xa[-1] + 5.0 * dxmax), ("damped", hub + 30.0),
                ("narrow", edge(1)), ("narrow", edge(2)), ("narrow", hub - 70.0), ("narrow", far_end()),
                ("medium", hub + 55.0), ("medium", hub - 20.0), ("medium", far_end()),
                ("broad", hub - 200.0 * dxmax), ("broad", hub + 150.0 * dxmax), ("broad", hub + 10.0),
                ("wide", rng.uniform(xa[0], xa[-1])), ("wide", rng.uniform(xa[0], xa[-1])), ("narrow", edge(ntile - 1))]
    assert len(plan) == K
    t = np.array([kinds[kind](c) for kind, c in plan])
    return t[rng.permutation(K)]


def classes(x, t, f32=False):
    """The kernel's predicates (ff_classify_batch) for every (line, full tile): arrays [K, tiles] of far, deep, mid, wide."""
    ntile = x.size // TILE
    lo, hi = x[TILE * np.arange(ntile)], x[TILE * np.arange(ntile) + TILE - 1]
    mid, half = 0.5 * (lo + hi), 0.5 * np.abs(hi - lo)
    c, L, G = t[:, 1, None], t[:, 2, None], t[:, 3, None]
    s, y = 2.0 * vo.SQRT_LN2 / G, L * vo.SQRT_LN2 / G
    zone = lambda r2: np.sqrt(np.maximum(r2 - y * y, 0.0)) / s
    dist = np.abs(mid[None, :] - c) - half[None, :]
    beyond = dist >= FF_DIST * half[None, :]
    far = beyond & (dist >= zone(MID_Z2 if f32 else 64.0))
    deep = far & (dist < zone(625.0))
    midc = beyond & (dist >= zone(MID_Z2)) & ~far
    tile_span = TILE * np.max(np.abs(np.diff(x)))
    wide = (s * (0.5 * tile_span) <= WIDE_MAX) & ~far
    return far, deep, midc, wide


@functools.lru_cache(maxsize=None)
def case(name, K):
    """Grid, data, the W walkers and the oracle's log-posterior of one (shape, K): computed once, shared, read-only."""
    x = grid(name)
    t = lines(name, K)
    rng = np.random.default_rng(7)
    noise = np.full(x.size, SD)
    pad = 50.0 * np.max(np.abs(np.diff(x)))
    bounds = np.array([[x.min() - pad, x.max() + pad, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=vo.MODE_VOIGT4, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    flux = vo.model_flux(vo.Region(x=x, flux=np.ones(x.size), noise=noise, **kw), t.reshape(-1)) + rng.normal(0, SD, x.size)
    reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
    th = np.empty((W, 4 * K))
    for w in range(W):          # walker w: the lines rotated by w places; walker 0 exact, the others moved by 1e-4
        tw = t * (1.0 + (1e-4 if w else 0.0) * rng.standard_normal(t.shape))
        th[w] = np.roll(tw, w % K, axis=0).reshape(-1)
    want = vo.log_prob_batch_fast(reg, th)
    for a in (x, flux, noise, th, want, bounds):
        a.setflags(write=False)
    return dict(x=x, flux=flux, noise=noise, th=th, want=want, bounds=bounds, reg=reg, t=t)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_cover_every_class(name, K):
    c = case(name, K)
    assert np.isfinite(c["want"]).all()
    far, deep, midc, wide = classes(c["x"], c["t"])
    near = ~(far | midc | wide)
    assert far.any() and near.any()
    if K >= 7:
        assert deep.any() and (far & ~deep).any() and midc.any() and wide.any()
    if K == 16:
        for f32 in (False, True):
            nfar = classes(c["x"], c["t"], f32)[0].sum(0)
            assert nfar.min() <= 8 < nfar.max(), (f32, nfar)


def _context(dtype, packing, c, K):
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0, dtype=vamp_amd.F64 if dtype == "f64" else vamp_amd.F32)
    ctx.set_packing(packing)       # 256 forced: regions below 2048 px would not take it on their own
    ctx.set_regions(c["x"], c["flux"], c["noise"], K, mode=vamp_amd.MODE_VOIGT4, bounds=c["bounds"])
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("packing", [256, 64])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lnprob_matches_oracle(dtype, packing, name, K):
    c = case(name, K)
    want = c["want"]
    with _context(dtype, packing, c, K) as ctx:
        got = ctx.lnprob(c["th"])
    assert np.isfinite(want).all() and np.isfinite(got).all()
    if dtype == "f64":
        err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
        print(f"{dtype} pack {packing} {name} K={K}: |lnprob| ~ {np.abs(want).mean():.3e}, worst error {err:.2e}")
        assert err <= 1e-9
    else:
        err = np.max(np.abs(got - want) / np.abs(want))
        print(f"{dtype} pack {packing} {name} K={K}: |lnprob| ~ {np.abs(want).mean():.3e}, worst error {err:.2e}")
        assert err <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("packing", [256, 64])
def test_stretch_steps_match_oracle(packing):
    """P = 2304, K = 7 (wavefronts with 3 / 2 / 2 / 2 tiles): five stretch-move steps against the oracle's sampler."""
    c = case("P2304", 7)
    fn = lambda q: vo.log_prob_batch_fast(c["reg"], q)
    with _context("f64", packing, c, 7) as ctx:
        ctx.sampler_init(c["th"], seed=2304, a=2.0, split_block=W)
        res = ctx.run(5)
    chain, lchain, nacc = vo.run_sampler(fn, c["th"], c["want"], 5, seed=2304, block=W)
    assert np.array_equal(res["n_accept"], nacc)
    assert np.allclose(res["chain"], chain, rtol=1e-10, atol=1e-12)
    assert np.allclose(res["lnprob"], lchain, rtol=1e-9, atol=1e-9)
