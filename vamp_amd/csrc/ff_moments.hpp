// Per-context data moments of the full 256-pixel tiles (k_tile_tables) and the guard of the moment form of a tile's
// chi^2 (sweep_range_ff).  Compiled into the kernels and, through tests/host/ff_moments_host.cpp, on the host.
//
// A tile without a near line has the model flux m = 1 - a with a the tile's interpolant alone, a polynomial b_q on each
// quarter q of the tile in the pixel's place u.  Its chi^2 is then a quadratic form in b on moments of the data:
//     sum w^2 ((f - 1) + a)^2 = C0 + 2 sum_q b_q.S_q + sum_q b_q' Q_q b_q
//     S_q[j] = sum w^2 (f - 1) u^j (j = 0..13),   Q_q[n] = sum w^2 u^n (n = 0..26),   C0 = sum w^2 (f - 1)^2,
// quarters in coefficient order (ascending abscissa), so that the grid's orientation drops out.
#pragma once
#include "voigt_math.hpp"

namespace vamp {

// layout of one tile's moments, in doubles: Q[4][FFM_QROW] (27 moments and one spare slot per quarter), then S[4][14].
// The spare slots hold what the guard needs: sqrt(C0) and sqrt(sum_q Q_q[0]), and C0 itself.
constexpr int FFM_NS = 14, FFM_NQ = 27, FFM_QROW = 28;
constexpr int FFM_S = 4 * FFM_QROW;                 // offset of S
constexpr int FFM_TILE = FFM_S + 4 * FFM_NS;        // 168 doubles per tile
constexpr int FFM_C0 = 0 * FFM_QROW + FFM_NQ;       // spare slot of quarter 0: C0
constexpr int FFM_RC = 1 * FFM_QROW + FFM_NQ;       // ... of quarter 1: sqrt(C0)
constexpr int FFM_RQ = 2 * FFM_QROW + FFM_NQ;       // ... of quarter 2: sqrt(Q_0[0] + Q_1[0] + Q_2[0] + Q_3[0])

// The node record (VAMP_TILE_MOMENTS == 2, the default): the same chi^2 written on the values a_n of the absorption at the
// tile's 16 Chebyshev nodes instead of the series they are transformed into.  The tile's interpolant is
// a(x) = sum_n l_n(t(x)) a_n with l_n the Lagrange basis of the nodes t_n on t = (x - mid) / half, so
//     sum w^2 ((f - 1) + a)^2 = C0 + sum_n a_n (2 S'_n + sum_m Q'_nm a_m),
//     S'_n = sum w^2 (f - 1) l_n,   Q'_nm = sum w^2 l_n l_m   (symmetric; sum_nm Q'_nm = sum w^2 since sum_n l_n = 1).
// The node abscissae are mid + half t_n whatever the grid's orientation, so the record needs no quarters.
// Layout of one tile, in doubles: Q'[16][16] row by row, S'[16], then C0, sqrt(C0), sqrt(sum w^2); padded to whole
// 64-byte lines (lane 16 g + n reads columns 4 g .. 4 g + 3 of row n: 32 aligned bytes).
constexpr int FFN_NODES = 16;
constexpr int FFN_Q = 0;
constexpr int FFN_S = FFN_NODES * FFN_NODES;        // offset of S'
constexpr int FFN_C0 = FFN_S + FFN_NODES;           // C0
constexpr int FFN_RC = FFN_C0 + 1;                  // sqrt(C0)
constexpr int FFN_RQ = FFN_C0 + 2;                  // sqrt(sum w^2)
constexpr int FFN_TILE = 280;                       // doubles per tile
static_assert(FFN_TILE >= FFN_RQ + 1 && FFN_TILE % 8 == 0, "the record fits, and a tile starts on a 64-byte line");

// The moment form is a sum with cancellation: its terms are bounded by M = (sqrt(C0) + amax sqrt(sum_q Q_q[0]))^2 with amax
// the largest |a| at the tile's nodes (Cauchy-Schwarz on sum w^2 (|f - 1| + |a|)^2), and its rounding error is about
// FFM_ULPS 2^-53 M.  A tile takes the moment form only if that is at most FFM_BOUND = 2^-40 x 256: 1e-12 of the chi^2 of a
// fitted tile.  Both sides are powers of two times M, so the rule is r = sqrt(C0) + amax sqrt(sum Q_q[0]) <= FFM_RMAX = 2^9
// exactly (squaring is monotonic and 2^18 is exact).  Data with weights of 1e10 (the zero-residual suites, which need chi^2
// to a pixel's rounding) have sqrt(sum Q) ~ 1e11 and never qualify.  NaN compares false.
constexpr double FFM_ULPS = 8.0;
constexpr double FFM_BOUND = 256.0 / 1099511627776.0;          // 2^-40 x 256
constexpr double FFM_RMAX = 512.0;                             // sqrt(FFM_BOUND 2^53 / FFM_ULPS)
VAMP_DEV bool ff_moments_ok(double root_c0, double root_q0, double amax) {
    return fma(amax, root_q0, root_c0) <= FFM_RMAX;
}
// Asked BEFORE the node stage, of the data alone: is the tile worth trying?  ff_moments_ok with amax = 0 is necessary; and
// where the model fits the data, sqrt(C0) / sqrt(sum Q_q[0]) is the r.m.s. absorption of the tile, which amax cannot be
// below, so a tile with 2 sqrt(C0) > FFM_RMAX would fail the rule after the node stage and pay for that stage twice (deep
// tiles of wide lines).  Turning a tile away here costs speed at most, never a digit: it is swept pixel by pixel.
VAMP_DEV bool ff_moments_try(double root_c0, double root_q0) {
    return ff_moments_ok(root_c0, root_q0, 0.0) && root_c0 + root_c0 <= FFM_RMAX;
}

}  // namespace vamp
