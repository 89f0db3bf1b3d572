// Predicates of a (line record, tile) pair that the far-field classification decides once per pair, so that the tile
// loop need not derive them from the pixels.  Pure functions of (c, s, y) of the line and (mid, half) of the tile as
// the context's tile table holds them; compiled into the kernels and, through tests/host/ff_pred_host.cpp, on the host.
#pragma once
#include "voigt_math.hpp"

namespace vamp {

// margin of ff_tile_in_zone below R2_CORE, relative
constexpr double FF_ZONE_MARGIN = 1.0 / 1024.0;

// true: EVERY pixel of the tile [mid - half, mid + half] has r2 = fma(X, X, y y) < R2_CORE with X = |x - c| s (or its
// minimum with a cap), as tile_voigt computes them -- the whole tile lies in the zone of the line's Taylor table.
// Why the margin is enough: |x - c| <= |mid - c| + half + e, where e is the rounding of the table's mid = (x_lo + x_hi) / 2,
// half an ulp of mid.  The sum below, its product with s and the pixel's own two roundings move X by 5 ulps in all, r2 by
// 12; e is below half / 4096 on any grid whose neighbouring abscissae are 16 ulps apart (half spans 127.5 spacings).
// Together far less than the margin's 2^-11 of X.  The price: a tile whose farther edge lies in 7.996 <= |z| < 8 is
// left to the pixels' own votes, which cost what they cost before.  NaN compares false.
VAMP_DEV bool ff_tile_in_zone(double c, double s, double y, double mid, double half) {
    const double Xf = (fabs(mid - c) + half) * s;
    return fma(Xf, Xf, y * y) < R2_CORE * (1.0 - FF_ZONE_MARGIN);
}

}  // namespace vamp
