"""The guards of the far-field node evaluation (ff_eval2: the clamp at X_FAR with its voigt_far patch, the e^{-x^2} patch
for y < Y_TINY) are compiled into one copy of the tile loop only; staging decides per walker which copy runs
(ff_guard_bits).  A walker that needs the clamp and does not get it must be SEEN to fail, so the planted line here is one
for which the unguarded loop has no finite answer:

  G = 1e-40, L = 1e-41: s = 2 sqrt(ln 2) / G = 1.7e40 per unit of x, y = 0.083.  Every Chebyshev node of every far tile is
  at least 2 half-widths of a tile from the centre, so X > 1e42 there and the denominators of the pair form of the
  continued fraction (voigt_jfrac_x2<2>: a product of X^8 terms) overflow: inf * 0 = NaN.  The CPU half shows that with
  the host build of the very functions (tests/host/voigt_host.cpp): the pair form is non-finite at every node, voigt_far
  is finite and equals scipy's wofz to 1e-13.  A walker holding this line gets a NaN from the unguarded loop, a finite
  lnprob within the fp64 bar of the oracle from the guarded one: the GPU half asserts the latter for VOIGT4, NBZ3 (there
  the line's L is the region's, so y = 6e39: the fraction overflows through y as well) and a free sd, under both packings,
  for lnprob and two sampler steps.  The NBZ3 case failed on its first GPU run (lnprob -inf for a planted walker,
  workgroup per walker): the guarded ff_eval2 clamped X but not y, and the overflowing denominator reached the OTHER
  line of the slot pair through the reciprocal the two share (ff_frac2), which no patch replaces.  ff_eval2 now bounds
  both coordinates.

  The older planted "reach" line of test_gpu_tile_tables.py (G = 0.05, X ~ 5e4) sets the bit but cannot show a missing
  one: the CPU half evaluates the unguarded pair form there and prints its error against wofz (rounding level).

Threshold walkers: y one ulp below Y_TINY and at it, a reach product s max(|x_first - c|, |x_last - c|) at X_FAR and one
ulp above, on ascending and descending grids, with the centre inside the region and beyond either end.  G is a power of
two, so the device's reciprocal of G is exact and the numpy predicate (test_gpu_tile_tables.guard_bits) rounds as the
device formula does; the CPU half asserts the classification, the GPU half only the oracle bar (the two copies of the
loop agree to the bit wherever the guard is not needed, so nothing more can be seen there).

No lnprob-level test of the y < Y_TINY patch is possible: it adds sqrt(pi) e^{-x^2} at a far node, |z| >= 8, which is at
most 3e-28 of the line's peak.  This module claims no coverage of that patch's value, only of its bit.

Bar: that of tests/test_gpu_parity.py, |delta lnprob| <= 1e-9 max(1, |lnprob|); sampler positions to 1e-10 with identical
accept counts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
from scipy.special import wofz

from oracle import vamp_oracle as vo
import test_gpu_tile_tables as tt
import zero_residual as zr

TILE, W, SD = tt.TILE, tt.W, tt.SD
P, K = 2304, 7
PLANT_WALKERS, PLANT_SLOT = (5, 22, 41), 4
PLANT_L, PLANT_G = 1.0e-41, 1.0e-40
NBZ = np.array([0.7, 1215.67, 2.4e15, 4.0e10])            # l_fixed, line, x_origin, x_scale (tests/test_gpu_sweep_pixels.py)
PAD = 4000.0                                              # the centre prior reaches this far beyond the grid
MODES = {"voigt4": (vo.MODE_VOIGT4, False), "nbz3": (vo.MODE_NBZ3, False), "voigt4-sd": (vo.MODE_VOIGT4, True)}
NODES = np.cos(np.pi * (np.arange(16) + 0.5) / 16.0)      # the 16 Chebyshev nodes of a tile (ff_coefficients)


def _host():
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "libvoigt_host.so")
    if not os.path.exists(so):          # as tests/test_voigt_properties.py: the two CPU tests here must not depend on the test order
        import __graft_entry__ as ge
        ge.build()
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.voigt_jfrac_x2_host.argtypes = [C.c_int, C.c_int64, dp, dp, dp, dp, dp]
    lib.voigt_far_host.argtypes = [C.c_int64, dp, dp, dp]
    ptr = lambda a: a.ctypes.data_as(dp)

    def pair(M, X0, X1, y):
        X0, X1, y = (np.ascontiguousarray(np.broadcast_to(a, np.shape(X0)), dtype=np.float64) for a in (X0, X1, y))
        h0, h1 = np.empty_like(X0), np.empty_like(X0)
        lib.voigt_jfrac_x2_host(M, X0.size, ptr(X0), ptr(X1), ptr(y), ptr(h0), ptr(h1))
        return h0, h1

    def far(X, y):
        X, y = (np.ascontiguousarray(np.broadcast_to(a, np.shape(X)), dtype=np.float64) for a in (X, y))
        out = np.empty_like(X)
        lib.voigt_far_host(X.size, ptr(X), ptr(y), ptr(out))
        return out
    return pair, far


def far_nodes(x, c, G, L):
    """X of the line at the 16 nodes of every full tile it is far from (beyond 2 half-widths and outside |z| < 8)"""
    n = x.size // TILE
    lo, hi = x[TILE * np.arange(n)], x[TILE * np.arange(n) + TILE - 1]
    mid, half = 0.5 * (lo + hi), 0.5 * np.abs(hi - lo)
    s, y = 2.0 * vo.SQRT_LN2 / G, L * vo.SQRT_LN2 / G
    dist = np.abs(mid - c) - half
    far = (dist >= 2.0 * half) & (dist >= np.sqrt(max(64.0 - y * y, 0.0)) / s)
    assert far.any()
    return (np.abs(mid[far, None] + half[far, None] * NODES[None, :] - c) * s).ravel(), y


def _hub(x):
    xa = np.sort(x)
    return 0.5 * (xa[TILE] + xa[2 * TILE - 1]) + 40.0          # second tile, half way between two pixels


def test_unguarded_pair_form_has_no_finite_answer_for_the_planted_line():
    pair, far = _host()
    x = tt.make_grid(P, "up")
    X, y = far_nodes(x, _hub(x), PLANT_G, PLANT_L)
    assert X.min() > 1e40 and 0.05 < y < 0.1
    h0, h1 = pair(2, X, X[::-1].copy(), y)
    assert not np.isfinite(h0).any() and not np.isfinite(h1).any()
    got = far(X, y) / np.sqrt(np.pi)
    want = wofz(X + 1j * y).real
    assert np.isfinite(got).all() and (want > 0).all()
    assert np.max(np.abs(got - want) / want) <= 1e-13


def test_pair_form_at_the_older_reach_line_is_accurate_without_the_clamp():
    """G = 0.05, L = 0.01 (test_gpu_tile_tables.guard_case): X ~ 5e4 at the far end.  Recorded, and the reason why that
    line cannot show a missing reach bit."""
    pair, _ = _host()
    x = tt.make_grid(P, "up")
    X, y = far_nodes(x, _hub(x), 0.05, 0.01)
    assert X.max() > tt.X_FAR
    beyond = X > tt.X_FAR
    h0, _ = pair(2, X, X[::-1].copy(), y)
    want = np.sqrt(np.pi) * wofz(X + 1j * y).real
    err = np.abs(h0 - want) / want
    print("unguarded voigt_jfrac_x2<2> at the reach line: X up to %.3g, %d nodes beyond X_FAR, relative error against wofz "
          "%.2e there, %.2e over all far nodes" % (X.max(), beyond.sum(), err[beyond].max(), err.max()))
    assert np.isfinite(h0).all()


# ---- cases -----------------------------------------------------------------------------------------------------------
def _theta(t, mode):
    return zr.native_to_mode(t, mode, NBZ if mode == vo.MODE_NBZ3 else None)


def _make(kind, mode, sd, plant):
    """P = 2304, K = 7: the lines of test_gpu_tile_tables.make_lines, W rotated and slightly moved walkers; ``plant``:
    {walker: (slot, (A, c, L, G))}.  Returns a dict like tt.case's, with the mode's extras."""
    x = tt.make_grid(P, kind)
    rng = np.random.default_rng(P + 10 * mode + sd + len(kind))
    t = tt.make_lines(x, K, rng)
    if mode == vo.MODE_NBZ3:
        t[:, 2] = NBZ[0]
    noise = np.full(P, SD)
    bounds = np.array([[x.min() - PAD, x.max() + PAD, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=mode, sample_sd=sd, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    if mode == vo.MODE_NBZ3:
        kw.update(l_fixed=NBZ[0], line=NBZ[1], x_origin=NBZ[2], x_scale=NBZ[3])
    truth = np.append(_theta(t, mode), SD) if sd else _theta(t, mode)
    flux = vo.model_flux(vo.Region(x=x, flux=np.ones(P), noise=noise, **kw), truth) + rng.normal(0, SD, P)
    reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
    rows, native = [], []
    for w in range(W):
        tw = np.roll(t * (1.0 + (1e-4 if w else 0.0) * rng.standard_normal(t.shape)), w % K, axis=0)
        if w in plant:
            slot, line = plant[w]
            tw[slot] = line
            if mode == vo.MODE_NBZ3:
                tw[slot, 2] = NBZ[0]
        native.append(tw)
        row = _theta(tw, mode)
        rows.append(np.append(row, SD * rng.uniform(0.8, 1.5)) if sd else row)
    th = np.array(rows)
    want = vo.log_prob_batch_fast(reg, th)
    return tt._freeze(dict(x=x, flux=flux, noise=noise, th=th, want=want, bounds=bounds, reg=reg, K=K, native=np.array(native),
                           mode=mode, sd=sd))


@functools.lru_cache(maxsize=None)
def planted_case(name):
    mode, sd = MODES[name]
    c = _hub(tt.make_grid(P, "up"))
    return _make("up", mode, sd, {w: (PLANT_SLOT, (2.0, c, PLANT_L, PLANT_G)) for w in PLANT_WALKERS})


# threshold walkers: (what, G, which end the distance is measured from, +1: the centre lies toward / beyond the OTHER end)
def _ulps(v, n):
    for _ in range(abs(n)):
        v = np.nextafter(v, np.inf if n > 0 else -np.inf)
    return float(v)


def _reach_pair(x, G, from_first):
    """two centres one ulp apart: s max(|x_first - c|, |x_last - c|) <= X_FAR for the first, > X_FAR for the second"""
    s = 2.0 * vo.SQRT_LN2 / G
    a, b = (x[0], x[-1]) if from_first else (x[-1], x[0])           # the distance that counts is the one from a
    sign = 1.0 if b > a else -1.0
    prod = lambda c: s * max(abs(x[0] - c), abs(x[-1] - c))
    c0 = a + sign * tt.X_FAR / s
    cs = [_ulps(c0, sign_n) for sign_n in range(-6, 7)]
    cs.sort(key=prod)
    below = [c for c in cs if prod(c) <= tt.X_FAR]
    above = [c for c in cs if prod(c) > tt.X_FAR]
    assert below and above and abs(x[-1 if from_first else 0] - below[-1]) < abs(a - below[-1])
    return below[-1], above[0]


def _tiny_pair(G):
    """two L one ulp apart: y = (L sqrt(ln 2)) / G one step below Y_TINY (bit set) and at or above it (bit clear)"""
    y = lambda L: (L * vo.SQRT_LN2) / G
    Ls = sorted(_ulps(tt.Y_TINY * G / vo.SQRT_LN2, n) for n in range(-6, 7))
    below = [L for L in Ls if y(L) < tt.Y_TINY]
    above = [L for L in Ls if y(L) >= tt.Y_TINY]
    assert below and above and y(below[-1]) == np.nextafter(tt.Y_TINY, 0.0)
    return below[-1], above[0]


@functools.lru_cache(maxsize=None)
def threshold_case(kind):
    x = tt.make_grid(P, kind)
    plant, expect = {}, {}
    w = 3
    L_lo, L_hi = _tiny_pair(64.0)
    for L, bit in ((L_lo, True), (L_hi, False)):
        plant[w], expect[w] = (1, (1.5, _hub(x), L, 64.0)), (bit, False)
        w += 5
    # G = 1/4: the centre lies inside the region; G = 1/2: beyond the other end (span 2303 < X_FAR / s = 3003)
    for G in (0.25, 0.5):
        for from_first in (True, False):
            for c, bit in zip(_reach_pair(x, G, from_first), (False, True)):
                inside = x.min() < c < x.max()
                assert inside == (G == 0.25)
                plant[w], expect[w] = (PLANT_SLOT, (2.0, c, 0.01, G)), (False, bit)
                w += 5
    assert w - 5 < W
    return _make(kind, vo.MODE_VOIGT4, False, plant), expect


def device_guard_bits(x, native):
    """ff_guard_bits with the staging's arithmetic (one reciprocal of G, then two products), per walker"""
    c, L, G = native[:, :, 1], native[:, :, 2], native[:, :, 3]
    rG = 1.0 / G
    s, y = (2.0 * vo.SQRT_LN2) * rG, (L * vo.SQRT_LN2) * rG
    reach = s * np.maximum(np.abs(x[0] - c), np.abs(x[-1] - c))
    return (~(y >= tt.Y_TINY)).any(1), (~(reach <= tt.X_FAR)).any(1)


@pytest.mark.parametrize("kind", ["up", "down"])
def test_threshold_walkers_are_classified_as_the_device_would(kind):
    g, expect = threshold_case(kind)
    assert np.isfinite(g["want"]).all()
    assert sorted(set(expect.values())) == [(False, False), (False, True), (True, False)]
    tiny, reach = tt.guard_bits(g["x"], g["th"], K)
    dtiny, dreach = device_guard_bits(g["x"], g["native"])
    for w in range(W):
        want = expect.get(w, (False, False))
        assert (tiny[w], reach[w]) == want == (dtiny[w], dreach[w]), (kind, w, want, tiny[w], reach[w], dtiny[w], dreach[w])


@pytest.mark.parametrize("name", list(MODES))
def test_planted_walkers_set_the_reach_bit_and_the_oracle_is_finite(name):
    g = planted_case(name)
    assert np.isfinite(g["want"]).all()
    _, reach = device_guard_bits(g["x"], g["native"])
    assert [w for w in range(W) if reach[w]] == list(PLANT_WALKERS)
    line = g["native"][PLANT_WALKERS[0], PLANT_SLOT]
    assert g["x"].min() < line[1] < g["x"].max() and np.min(np.abs(g["x"] - line[1])) > 0.25       # between two pixels


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _context(packing, g):
    import vamp_amd
    ctx = vamp_amd.HipContext(device=0)
    ctx.set_packing(packing)
    ctx.set_regions(g["x"], g["flux"], g["noise"], K, mode=g["mode"], sample_sd=g["sd"], bounds=g["bounds"],
                    nbz=NBZ[None, :] if g["mode"] == vo.MODE_NBZ3 else None)
    return ctx


def _bar(got, want, what):
    assert np.isfinite(want).all() and np.isfinite(got).all(), (what, np.flatnonzero(~np.isfinite(got)))
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("%s: |lnprob| ~ %.3e, worst error %.2e at walker %d (bar 1e-9)" % (what, np.abs(want).mean(), err.max(), err.argmax()))
    assert err.max() <= 1e-9, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("packing", tt.PACKINGS)
def test_planted_line_lnprob_and_two_steps(packing, name):
    g = planted_case(name)
    with _context(packing, g) as ctx:
        got = ctx.lnprob(g["th"])
        ctx.sampler_init(g["th"], seed=P + packing, a=2.0, split_block=W)
        res = ctx.run(2)
    _bar(got, g["want"], "planted %s packing %d" % (name, packing))
    fn = lambda q: vo.log_prob_batch_fast(g["reg"], q)
    chain, lchain, nacc = vo.run_sampler(fn, g["th"], g["want"], 2, seed=P + packing, block=W)
    assert np.isfinite(res["lnprob"][-1]).all()
    assert np.array_equal(res["n_accept"], nacc)
    assert np.allclose(res["chain"], chain, rtol=1e-10, atol=1e-12)
    assert np.allclose(res["lnprob"], lchain, rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["up", "down"])
@pytest.mark.parametrize("packing", tt.PACKINGS)
def test_threshold_walkers_match_oracle(packing, kind):
    g, _ = threshold_case(kind)
    with _context(packing, g) as ctx:
        got = ctx.lnprob(g["th"])
    _bar(got, g["want"], "thresholds %s packing %d" % (kind, packing))
