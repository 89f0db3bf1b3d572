"""The Taylor table in the in-zone path of the fp64 far-field loop (table_eval_tile: one pixel at a time as built, two at a
time -- table_eval2 -- with -DVAMP_TAB_PAIR=1) on the GPU: the log-posterior against the oracle at the bar of
tests/test_gpu_parity.py, 1e-9 max(1, |lnprob|).

P = 4096, K = 2.  A lane holds pixels 64 apart, and table_eval2 takes them as (0, 1) and (2, 3).  Line 0 has
s = 2 sqrt(ln 2) / G = 1 / 64 and its centre on a pixel, so that in a tile inside its table zone

  * every 32nd pixel sits on an interval border of the table (2 X an integer, to the rounding of s), where either
    neighbouring row is right, and
  * the two pixels of every pair are a whole unit of X apart: each pair reads two different rows.

The same line is near but NOT in the zone for tile 3 (its farther edge lies beyond |z| = 8), so tile_voigt is still taken
beside the table path.  Other walkers move the centre by fractions of a pixel, halve the scale (pairs that share a row
or straddle one border) and swap the lines' slots.  What each walker is for is asserted on the CPU (the classification's
rules and the predicate's host build, tests/test_gpu_ff_zone.py) before anything runs."""
import functools

import numpy as np
import pytest

from oracle import vamp_oracle as vo
import test_gpu_ff_zone as fz

P, K, W, SD, TILE = 4096, 2, 16, 0.05, 256
G64 = 128.0 * vo.SQRT_LN2             # s = 1 / 64
HOME = 5                              # the tile that holds line 0's centre


@functools.lru_cache(maxsize=None)
def case():
    x = np.arange(P, dtype=np.float64) - (P - 1) / 2.0
    rng = np.random.default_rng(64)
    c0 = x[TILE * HOME + 10]
    far_line = (1.5, 0.5 * (x[TILE * 12] + x[TILE * 13 - 1]) + 7.0, 0.4, 8.0)
    native = np.empty((W, K, 4))
    for w in range(W):
        G = G64 * (2.0 if w % 4 == 3 else 1.0)                    # s = 1 / 128: the pixels of a pair half a unit apart
        dc = 0.0 if w % 4 == 0 else rng.uniform(-0.5, 0.5)          # off the pixel: borders fall between pixels
        L = 0.5 if w < 8 else 1e-3 * G
        near_line = (2.0 + 0.1 * w, c0 + dc, L, G)
        native[w] = (near_line, far_line) if w % 2 == 0 else (far_line, near_line)
    th = native.reshape(W, -1).copy()
    noise = np.full(P, SD)
    bounds = np.array([[x.min() - 50.0, x.max() + 50.0, 1.0e5, 1.0e5]])
    kw = dict(n_comp=K, mode=vo.MODE_VOIGT4, c_lo=bounds[0, 0], c_hi=bounds[0, 1], sigma_max=1.0e5, fwhm_max=1.0e5)
    flux = vo.model_flux(vo.Region(x=x, flux=np.ones(P), noise=noise, **kw), th[0]) + rng.normal(0, SD, P)
    reg = vo.Region(x=x, flux=flux, noise=noise, **kw)
    want = vo.log_prob_batch_fast(reg, th)
    for a in (x, flux, noise, th, want, bounds, native):
        a.setflags(write=False)
    return dict(x=x, flux=flux, noise=noise, th=th, want=want, bounds=bounds, native=native)


def test_case_is_what_it_is_for():
    c = case()
    x, nat = c["x"], c["native"]
    near, zone = fz.routes(c)                                       # [W, K, tiles]
    # walker 0, line 0: in the zone for its own tile and both neighbours, near but outside it for tile 3
    assert (near[0, 0, [4, 5, 6]] & zone[0, 0, [4, 5, 6]]).all()
    assert near[0, 0, 3] and not zone[0, 0, 3]
    # every walker has tiles in the zone, in either slot; at s = 1 / 64 also a near tile outside it (at 1 / 128 the tiles
    # beyond the zone are the interpolant's)
    for w in range(W):
        k = w % 2
        assert (near[w, k] & zone[w, k]).any(), w
        assert (near[w, k] & ~zone[w, k]).any() or w % 4 == 3, w
    s = 2.0 * vo.SQRT_LN2 / nat[0, 0, 3]
    assert abs(s * 64.0 - 1.0) < 4 * 2.0 ** -53
    px = x[TILE * HOME:TILE * (HOME + 1)]
    X2 = 2.0 * np.abs(px - nat[0, 0, 1]) * s
    on_border = np.abs(X2 - np.round(X2)) < 1e-13
    assert on_border.sum() == 8                                     # every 32nd pixel
    row = np.floor(2.0 * np.abs(px - nat[0, 0, 1]) * s + 1e-9).reshape(4, 64)          # [pixel of the lane, lane]
    assert (row[0] != row[1]).all() and (row[2] != row[3]).all()    # both pairs of every lane straddle rows
    # ... and at half the scale some pairs share a row and some straddle one border
    s3 = 2.0 * vo.SQRT_LN2 / nat[3, 1, 3]
    row3 = np.floor(2.0 * np.abs(px - nat[3, 1, 1]) * s3).reshape(4, 64)
    same = row3[0] == row3[1]
    assert same.any() and (~same).any()


@pytest.mark.gpu
@pytest.mark.parametrize("packing", [0, 256])
def test_lnprob_matches_oracle(packing):
    import vamp_amd
    c = case()
    with vamp_amd.HipContext(device=0) as ctx:
        ctx.set_packing(packing)
        ctx.set_regions(c["x"], c["flux"], c["noise"], K, mode=vamp_amd.MODE_VOIGT4, bounds=c["bounds"])
        got = ctx.lnprob(c["th"])
    want = c["want"]
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"pack {packing}: |lnprob| ~ {np.abs(want).mean():.3e}, worst error {err.max():.2e} (walker {int(err.argmax())})")
    assert err.max() <= 1e-9
