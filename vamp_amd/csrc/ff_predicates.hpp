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

// A line "distant" from a super-tile -- the four adjacent tiles of a batch, [Mid - Half, Mid + Half] from the outer edges
// of its first and last tile: its centre lies >= VAMP_SUPER_DIST super-tile half-widths beyond the super-tile's edge, and
// the edge bound of r2 there is at least VAMP_FF_R2_M3, so that no point of the super-tile asks for a fraction deeper than
// 3 levels.  Such a line is evaluated once at the 16 Chebyshev nodes of the SUPER-tile and interpolated to the tiles' own
// nodes (VAMP_SUPER_NODES).  The factor is the distance from which a 16-node interpolant reproduces a wing to 4e-15
// (tests/test_ff_matrix.py); from 2 half-widths it holds only 6e-13, more than the node sums' bar allows.  Every tile of
// the super-tile lies inside it, so the line is at least as far from each tile, in units of the tile's own half-width
// too: distant implies the per-tile far predicate wherever r2 >= 300 > 64 does.  NaN compares false.
#ifndef VAMP_SUPER_DIST
#define VAMP_SUPER_DIST 4.0
#endif
#ifndef VAMP_FF_R2_M3
#define VAMP_FF_R2_M3 300.0
#endif
VAMP_DEV bool ff_super_distant(double c, double s, double y, double Mid, double Half) {
    const double distS = fabs(Mid - c) - Half;
    const double Xe = distS * s;
    return (distS >= VAMP_SUPER_DIST * Half) & (fma(Xe, Xe, y * y) >= VAMP_FF_R2_M3);
}
// the edge bound of a distant line: r2 >= this at every point of the super-tile (the depth of its fraction, 3 or 2 levels)
VAMP_DEV double ff_super_r2e(double c, double s, double y, double Mid, double Half) {
    const double Xe = (fabs(Mid - c) - Half) * s;
    return fma(Xe, Xe, y * y);
}
// (Mid, Half) of the super-tile whose first and last tile are (mid0, half0) and (mid3, half3), on either direction of the grid
VAMP_DEV void ff_super_tile(double mid0, double half0, double mid3, double half3, double& Mid, double& Half) {
    const double lo = fmin(mid0 - half0, mid3 - half3), hi = fmax(mid0 + half0, mid3 + half3);
    Mid = 0.5 * (lo + hi);
    Half = 0.5 * (hi - lo);
}

// The order of a batch's distant lines (bits of `dist`; d3 <= dist: the edge bound is below VAMP_FF_R2_M2, three levels):
// the three-level lines first, by ascending index inside a class, four bits each, first line in the lowest nibble.  The
// distant pass takes eight of them per iteration -- slot 4 t + g of iteration i is line 8 i + 4 t + g of the sequence --
// `iters` iterations in all, the first `iters3` of them at three levels (an iteration that holds one such line).
struct SuperOrder {
    unsigned long long seq;
    int n, iters, iters3;
};
VAMP_DEV SuperOrder super_order(unsigned dist, unsigned d3) {
    SuperOrder o;
    const unsigned cls[2] = {d3 & dist, dist & ~d3};
    unsigned long long seq = 0ull;
    int sh = 0;
    for (int c = 0; c < 2; ++c)
        for (unsigned m = cls[c]; m; m &= m - 1u) {
            seq |= (unsigned long long)__builtin_ctz(m) << sh;
            sh += 4;
        }
    o.seq = seq;
    o.n = sh >> 2;
    o.iters = (o.n + 7) >> 3;
    o.iters3 = (__builtin_popcount(cls[0]) + 7) >> 3;
    return o;
}

// The order in which the node pass of a full batch (ff_node_pass) evaluates the batch's far lines.  The sets are nested,
// n6 <= n4 <= n3 <= far (bit k: line k needs a fraction of at least that many levels for some tile of the batch).  The
// lines go deepest class first -- 6, 4, 3, 2 levels -- and by ascending index inside a class; neighbours of that sequence
// form a pair, a pair runs at the depth of its FIRST member (an odd last line of a class pairs with the first line of the
// next class, at its own depth), and an odd last line of all pairs with itself.
//   seq       line indices, four bits each, first line in the lowest nibble; an odd last line stands twice
//   solo      bit of the line that pairs with itself, 0 when the count is even: the second slot of that pair adds nothing
//   pairs[d]  consecutive pairs to run at 6, 4, 3 and 2 levels (d = 0 .. 3)
struct NpOrder {
    unsigned long long seq;
    unsigned solo;
    int pairs[4];
};
VAMP_DEV NpOrder np_pair_order(unsigned far, unsigned n6, unsigned n4, unsigned n3) {
    NpOrder o;
    const unsigned cls[4] = {n6, n4 & ~n6, n3 & ~n4, far & ~n3};
    unsigned long long seq = 0ull;
    int sh = 0, last = 0;
    for (int c = 0; c < 4; ++c) {
        for (unsigned m = cls[c]; m; m &= m - 1u) {
            last = __builtin_ctz(m);
            seq |= (unsigned long long)last << sh;
            sh += 4;
        }
    }
    const bool odd = (sh & 4) != 0;
    if (odd) seq |= (unsigned long long)last << sh;
    o.seq = seq;
    o.solo = odd ? 1u << last : 0u;
    const int h6 = (__builtin_popcount(n6) + 1) >> 1, h4 = (__builtin_popcount(n4) + 1) >> 1, h3 = (__builtin_popcount(n3) + 1) >> 1,
              hf = (__builtin_popcount(far) + 1) >> 1;
    o.pairs[0] = h6, o.pairs[1] = h4 - h6, o.pairs[2] = h3 - h4, o.pairs[3] = hf - h3;
    return o;
}

}  // namespace vamp
