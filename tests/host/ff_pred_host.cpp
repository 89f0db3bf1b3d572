// Host build of vamp_amd/csrc/ff_predicates.hpp for tests/test_ff_predicates.py: the predicate itself, and r2 of a
// pixel with the tile loop's operations (near-line loop of sweep_range_ff, then tile_voigt).  Built with
// -ffp-contract=off: every fma below is one written out.  Test infrastructure only: the product never loads this.
#include "../../vamp_amd/csrc/ff_predicates.hpp"
#include <cstdint>

extern "C" void ff_tile_in_zone_host(int64_t n, const double* c, const double* s, const double* y, const double* mid, const double* half,
                                     uint8_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = vamp::ff_tile_in_zone(c[i], s[i], y[i], mid[i], half[i]) ? 1 : 0;
}
// largest r2 over the npix abscissae x[i * npix ..] of pair i, for a line with cap xcap[i]
extern "C" void tile_r2_max_host(int64_t n, int64_t npix, const double* x, const double* c, const double* s, const double* y, const double* xcap,
                                 double* out) {
    for (int64_t i = 0; i < n; ++i) {
        const double y2 = y[i] * y[i];
        double hi = 0.0;
        for (int64_t p = 0; p < npix; ++p) {
            const double X = fmin(fabs(x[i * npix + p] - c[i]) * s[i], xcap[i]);
            const double r2 = fma(X, X, y2);
            hi = r2 > hi || r2 != r2 ? r2 : hi;
        }
        out[i] = hi;
    }
}
