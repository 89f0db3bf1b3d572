"""k_tile_tables against a reference of its own output.  vamp_set_regions builds, once per context, the tables the far-field
sweep reads: geo[(pix_off + base) >> 8] = (mid, +-half) of every full tile, and u[pix_off + i], the pixel's place in
its quarter of the tile.  The test hook vampdbg_tile_tables copies them out; a numpy restatement says what they must be.

geo: mid = 0.5 (x_lo + x_hi) and half = 0.5 |x_hi - x_lo| are each ONE exactly rounded addition (the halving is exact),
     so the table is bit-equal to numpy's, with the sign of half telling the grid's orientation.  fp32 contexts: x_lo and
     x_hi are the float-rounded abscissae converted to double.
u:   exact value, in numpy.longdouble: (x_i - (mid + half (q / 2 - 3 / 4))) 4 / half, q the pixel's quarter in ascending
     order of x, from the abscissae and the geometry in the context's precision (fp32: xf, (float)mid, (float)half).
     The device computes centre = fma(half, q / 2 - 3 / 4, mid), d = x_i - centre, u = d (4 rcp(half)):
       - the fma and the subtraction round once each, both results are at most max |x| of the tile in magnitude: the
         numerator is off by at most ulp(max |x|), which the scale 4 / half carries into u;
       - the reciprocal is within an ulp of 1 / half (fp64: the hardware's seed and two Newton steps; fp32: v_rcp_f32,
         1 ulp), the product by 4 is exact, the last product rounds once: at most 1.5 ulp relative, that is 1.5 x 2^-52
         in fp64 and 1.5 x 2^-23 = 3 x 2^-24 in fp32; the bound allows 4 eps with eps = 2^-52 and 2^-24.
     |u - exact| <= ulp(max |x| of the tile) 4 / half + 4 eps |u|, eps = 2^-52 (fp64), 2^-24 (fp32; ulp in fp32).
tails (pixels past a region's last full tile, regions without one) hold 0; every slot and pixel of the buffers belongs to
at most one region (asserted on the reference), so equality everywhere shows that no workgroup wrote another region's.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_tile_tables as tt

TILE = tt.TILE
SIZES = (255, 256, 257, 511, 512, 2404)
SECOND = (512, 300)                     # a second set_regions on the same context, fewer pixels


def reference(xs, f32):
    """(geo [slots, 2] with NaN where no tile owns the slot, u exact [N] longdouble, bound [N]) of the regions xs"""
    N = sum(x.size for x in xs)
    geo = np.full((N // TILE + 1, 2), np.nan)
    u, bound = np.zeros(N, dtype=np.longdouble), np.zeros(N)
    eps = 2.0 ** -24 if f32 else 2.0 ** -52
    off = 0
    for x in xs:
        xd = x.astype(np.float32).astype(np.float64) if f32 else x
        for base in range(0, x.size - TILE + 1, TILE):
            lo, hi = xd[base], xd[base + TILE - 1]
            mid, half = 0.5 * (lo + hi), 0.5 * abs(hi - lo)
            slot = (off + base) >> 8
            assert np.isnan(geo[slot, 0]), "two tiles share a slot"
            geo[slot] = mid, half if hi > lo else -half
            t = np.arange(TILE) // 64
            q = (t if hi > lo else 3 - t).astype(np.longdouble)
            m, h = (np.float32(mid), np.float32(half)) if f32 else (mid, half)
            m, h = np.longdouble(m), np.longdouble(h)
            tile = xd[base:base + TILE].astype(np.longdouble)
            exact = (tile - (m + h * (q / 2 - np.longdouble(0.75)))) * 4 / h
            ulp = np.spacing(np.float32(np.abs(tile).max())) if f32 else np.spacing(float(np.abs(tile).max()))
            u[off + base:off + base + TILE] = exact
            bound[off + base:off + base + TILE] = float(ulp) * 4.0 / half + 4.0 * eps * np.abs(exact).astype(np.float64)
        off += x.size
    return geo, u, bound


def test_reference_places_every_pixel_inside_its_quarter():
    xs = [tt.make_grid(P, kind) for kind in ("up", "down", "steps") for P in SIZES]
    geo, u, bound = reference(xs, False)
    assert np.abs(u).max() <= 1.0 + 1e-12 and bound.max() < 1e-12       # |u| <= 1: a quarter is 2 / 4 of the tile's span
    assert np.isfinite(geo[:, 0]).sum() == sum(x.size // TILE for x in xs)


def _tables(ctx, N, f32):
    fn = ctx._lib.vampdbg_tile_tables
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    slots = N // TILE + 1
    u = np.full(N, np.nan, dtype=np.float32 if f32 else np.float64)
    geo = np.full((slots, 2), np.nan)
    n = fn(ctx._h, None if f32 else u.ctypes.data, u.ctypes.data if f32 else None, geo.ctypes.data)
    assert n == slots, (n, ctx._lib.vamp_last_error())
    return u, geo


def _set(ctx, xs):
    import vamp_amd
    bounds = np.array([[x.min() - 1.0, x.max() + 1.0, 1.0e5, 1.0e5] for x in xs])
    ctx.set_regions(list(xs), [np.ones(x.size) for x in xs], [np.ones(x.size) for x in xs], [1] * len(xs),
                    mode=vamp_amd.MODE_VOIGT4, bounds=bounds)


def _compare(ctx, xs, f32, what):
    N = sum(x.size for x in xs)
    u, geo = _tables(ctx, N, f32)
    want_geo, exact, bound = reference(xs, f32)
    owned = ~np.isnan(want_geo[:, 0])
    assert np.array_equal(geo[owned].view(np.uint64), want_geo[owned].view(np.uint64)), (what, "geo differs")
    full = bound > 0
    assert (u[~full] == 0).all(), (what, "a tail pixel is not 0")
    err = np.abs(u.astype(np.longdouble) - exact).astype(np.float64)
    worst = np.flatnonzero(full)[np.argmax(err[full] / bound[full])]
    print("%s: %d tiles, |u - exact| nearest its bound: %.3g (bound there %.3g)" % (what, owned.sum(), err[worst], bound[worst]))
    assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["up", "down", "steps"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_tables_match_their_reference(dtype, kind):
    import vamp_amd
    f32 = dtype == "f32"
    xs = [tt.make_grid(P, kind) + 3.0e3 * r for r, P in enumerate(SIZES)]       # (regions apart: |x| up to 1.6e4)
    with vamp_amd.HipContext(device=0, dtype=vamp_amd.F32 if f32 else vamp_amd.F64) as ctx:
        _set(ctx, xs)
        _compare(ctx, xs, f32, "%s %s" % (dtype, kind))
        xs2 = [tt.make_grid(P, kind) for P in SECOND]
        _set(ctx, xs2)
        _compare(ctx, xs2, f32, "%s %s, second set_regions" % (dtype, kind))
