// Host build of the distant pass's pieces (vamp_amd/csrc/ff_predicates.hpp: vamp::ff_super_distant, ff_super_r2e,
// ff_super_tile, super_order; ff_super.inc: the cosine table) for tests/test_super_nodes.py.  Test infrastructure only:
// the product never loads this.  With -DSUPER_NODES_MAIN the file is a stand-alone program that walks the same entry
// points (for a sanitizer build of the host code).
#include "../../vamp_amd/csrc/ff_predicates.hpp"
#define FF_SUPER_QUAL static
#include "../../vamp_amd/csrc/ff_super.inc"
#include <cstdint>

extern "C" void super_distant_host(int64_t n, const double* c, const double* s, const double* y, const double* Mid, const double* Half,
                                   uint8_t* distant, double* r2e) {
    for (int64_t i = 0; i < n; ++i) {
        distant[i] = vamp::ff_super_distant(c[i], s[i], y[i], Mid[i], Half[i]) ? 1 : 0;
        r2e[i] = vamp::ff_super_r2e(c[i], s[i], y[i], Mid[i], Half[i]);
    }
}
extern "C" void super_tile_host(int64_t n, const double* mid0, const double* half0, const double* mid3, const double* half3, double* Mid,
                                double* Half) {
    for (int64_t i = 0; i < n; ++i) vamp::ff_super_tile(mid0[i], half0[i], mid3[i], half3[i], Mid[i], Half[i]);
}
extern "C" void super_order_host(int64_t n, const uint32_t* dist, const uint32_t* d3, uint64_t* seq, int32_t* counts) {
    for (int64_t i = 0; i < n; ++i) {
        const vamp::SuperOrder o = vamp::super_order(dist[i], d3[i]);
        seq[i] = o.seq;
        counts[3 * i] = o.n, counts[3 * i + 1] = o.iters, counts[3 * i + 2] = o.iters3;
    }
}
extern "C" void super_table_host(double* out) {
    for (int i = 0; i < 256; ++i) out[i] = FF_SUPER_C[i];
}
extern "C" double super_dist_factor_host() { return VAMP_SUPER_DIST; }

#ifdef SUPER_NODES_MAIN
#include <cstdio>
int main() {
    double t[256], Mid, Half, r2e;
    uint8_t d;
    super_table_host(t);
    const double m0 = -1920.5, h0 = 127.5, m3 = -1152.5, h3 = 127.5, c = 1500.0, s = 0.05, y = 0.1;
    super_tile_host(1, &m0, &h0, &m3, &h3, &Mid, &Half);
    super_distant_host(1, &c, &s, &y, &Mid, &Half, &d, &r2e);
    uint32_t dist = 0xffffu, d3 = 0x00f0u;
    uint64_t seq;
    int32_t cnt[3];
    super_order_host(1, &dist, &d3, &seq, cnt);
    std::printf("%g %g %d %g %llx %d %d %d %g\n", Mid, Half, (int)d, r2e, (unsigned long long)seq, cnt[0], cnt[1], cnt[2], t[0]);
    return 0;
}
#endif
