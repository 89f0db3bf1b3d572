"""The far-field classification decides per (line, tile) pair whether the whole tile lies inside the line's Taylor-table
zone (vamp::ff_tile_in_zone, vamp_amd/csrc/ff_predicates.hpp); for such a pair the near-line loop of the fp64 tile
sweep evaluates the table at once instead of letting tile_voigt find that out from the pixels.  The table covers
|z|^2 < R2_CORE only, so a set bit must imply r2 < R2_CORE for EVERY pixel of the tile, with r2 rounded as the loop
rounds it.  Both are reached here through a host build (tests/host/ff_pred_host.cpp).

  (i)   set bit  =>  max over the tile's 256 pixels of r2 < 64: 1e5 random pairs (widths from one pixel to three regions,
        damping y from 1e-12 to 1e4, ascending and descending grids at offsets 0 and 5000, capped and uncapped lines)
        and planted pairs whose farther edge sits on |z| = 8, on the predicate's own border, one ulp to either side of
        each, with y within 1e-10 of 8 (where w8 = sqrt(64 - y^2) / s has lost its digits), y >= 8 and NaN;
  (ii)  the margin gives nothing away that matters: a pair whose farthest pixel has r2 < 64 (1 - 2 margin) has its bit set;
  (iii) both values occur, in the random draw and among the planted pairs alone."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

TILE = 256
R2_CORE = 64.0
MARGIN = 1.0 / 1024.0          # vamp::FF_ZONE_MARGIN
SQRT_LN2 = np.sqrt(np.log(2.0))
X_FAR = 1.0e4


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "tests", "host", "libff_pred_host.so")
    if not os.path.exists(so):
        import __graft_entry__ as ge
        ge.build()
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def evaluate(lib, x, c, s, y, xcap):
    """x: [n, 256] abscissae of each pair's tile.  Returns (bit, r2max) with the tile table's (mid, half)."""
    n = x.shape[0]
    x = np.ascontiguousarray(x, dtype=np.float64)
    c, s, y, xcap = (np.ascontiguousarray(np.broadcast_to(a, (n,)), dtype=np.float64) for a in (c, s, y, xcap))
    x_lo, x_hi = x[:, 0], x[:, -1]
    mid, half = 0.5 * (x_lo + x_hi), 0.5 * np.abs(x_hi - x_lo)          # k_tile_tables
    bit, r2 = np.zeros(n, dtype=np.uint8), np.empty(n)
    lib.ff_tile_in_zone_host(C.c_int64(n), _p(c), _p(s), _p(y), _p(mid), _p(half), _p(bit))
    lib.tile_r2_max_host(C.c_int64(n), C.c_int64(TILE), _p(x), _p(c), _p(s), _p(y), _p(xcap), _p(r2))
    return bit.astype(bool), r2


def tiles(n, rng):
    """n tiles: pixel spacing 0.01 .. 2, first abscissa near 0 or near 5000, every other one descending"""
    dx = 10.0 ** rng.uniform(-2, 0.3, n)
    x0 = np.where(rng.random(n) < 0.5, 5000.0, 0.0) + rng.uniform(-300, 300, n)
    x = x0[:, None] + dx[:, None] * np.arange(TILE)[None, :]
    x[1::2] = x[1::2, ::-1]
    return x, dx


def test_set_bit_implies_every_pixel_in_the_table_zone(lib):
    rng = np.random.default_rng(20)
    n_set = n_clear = n_tight = 0
    for _ in range(5):
        n = 20000
        x, dx = tiles(n, rng)
        G = dx * 10.0 ** rng.uniform(0.0, np.log10(3.0 * 16384), n)       # one pixel .. three regions
        y = 10.0 ** rng.uniform(-12, 4, n)
        s = 2.0 * SQRT_LN2 / G
        w8 = np.sqrt(np.maximum(R2_CORE - y * y, 0.0)) / s
        mid, half = 0.5 * (x[:, 0] + x[:, -1]), 0.5 * np.abs(x[:, -1] - x[:, 0])
        c = mid + rng.uniform(-1.5, 1.5, n) * (w8 + half)
        xcap = np.where(rng.random(n) < 0.5, X_FAR, np.inf)
        bit, r2 = evaluate(lib, x, c, s, y, xcap)
        bad = bit & ~(r2 < R2_CORE)
        assert not bad.any(), (np.flatnonzero(bad)[:5], r2[bad][:5])
        must = r2 < R2_CORE * (1.0 - 2.0 * MARGIN)
        assert bit[must].all(), ("margin wider than stated", np.flatnonzero(must & ~bit)[:5])
        n_set += int(bit.sum()); n_clear += int((~bit).sum()); n_tight += int((bit & (r2 > 0.9 * R2_CORE)).sum())
    assert n_set > 5000 and n_clear > 5000 and n_tight > 100, f"set {n_set}, clear {n_clear}, set with r2 > 57.6: {n_tight}"


def planted():
    """Rows (x[256], c, s, y, xcap, bit expected or None): the tile's farther edge at a chosen r2"""
    rows = []
    for x0, dx, down in ((0.0, 1.0, False), (5000.0, 0.05, False), (-700.0, 0.3, True), (5000.0, 1.0, True)):
        x = x0 + dx * np.arange(TILE)
        lo, hi = x[0], x[-1]
        if down:
            x = x[::-1].copy()
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        for G, y in ((40.0 * dx, 1e-3), (400.0 * dx, 0.5), (900.0 * dx, 7.0), (2.0e7 * dx, np.sqrt(64.0 - 1e-10)), (300.0 * dx, 1e-12)):
            s = 2.0 * SQRT_LN2 / G
            for r2_edge, want in ((R2_CORE, False), (R2_CORE * (1.0 - MARGIN), None), (R2_CORE * (1.0 - 3.0 * MARGIN), True),
                                  (R2_CORE * (1.0 + 1e-6), False)):
                X = np.sqrt(max(r2_edge - y * y, 0.0))
                far = X / s                              # |mid - c| + half = far: the farther edge sits at r2_edge
                if far < half:
                    continue                             # (no tile this wide in the line's z: the damped cases at y ~ 8)
                for side in (-1.0, 1.0):
                    c0 = mid + side * (far - half)
                    for ulps in (-1, 0, 1):
                        c = c0
                        for _ in range(abs(ulps)):
                            c = np.nextafter(c, np.inf if ulps > 0 else -np.inf)
                        for xcap in (np.inf, X_FAR):
                            rows.append((x, c, s, y, xcap, want))
        # never in the zone: y >= 8, NaN in any field, an infinite scale
        for c, s, y in ((mid, 1e-3, 8.0), (mid, 1e-3, 1e4), (np.nan, 1e-3, 1.0), (mid, np.nan, 1.0), (mid, 1e-3, np.nan), (mid, np.inf, 1.0)):
            rows.append((x, c, s, y, np.inf, False))
        # always: the line's centre in the tile, |z| < 8 reaching far beyond it
        rows.append((x, mid + 3.0 * dx, 2.0 * SQRT_LN2 / (500.0 * dx), 0.1, np.inf, True))
    return rows


def test_planted_borders(lib):
    rows = planted()
    x = np.array([r[0] for r in rows])
    c, s, y, xcap = (np.array([r[i] for r in rows]) for i in (1, 2, 3, 4))
    bit, r2 = evaluate(lib, x, c, s, y, xcap)
    bad = bit & ~(r2 < R2_CORE)
    assert not bad.any(), [(rows[i][1:5], r2[i]) for i in np.flatnonzero(bad)[:5]]
    want = np.array([-1 if r[5] is None else int(r[5]) for r in rows])
    wrong = np.flatnonzero((want >= 0) & (bit.astype(int) != want))
    assert wrong.size == 0, [(rows[i][1:6], bool(bit[i]), r2[i]) for i in wrong[:5]]
    border = want < 0
    counts = (int((want == 1).sum()), int((want == 0).sum()), int(bit[border].sum()), int((~bit[border]).sum()))
    assert min(counts) > 0, f"planted: expected set {counts[0]}, expected clear {counts[1]}, on the border set {counts[2]} / clear {counts[3]}"
