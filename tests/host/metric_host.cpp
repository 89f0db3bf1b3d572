// Stand-alone host program for tests/test_metric.py: the argument checks, the output layout and the launch plan of
// vamp_amd/csrc/metric_host.hpp as metric.hip compiles them.  It prints "plan D waves lds_bytes" for every D, runs the
// checks on good and bad arguments -- the limits of n_mat, ld and the dimensions included, where a careless sum would
// overflow -- and ends with "checks ok", or says which expectation failed and returns 1.
// Built with -fsanitize=address,undefined by plain g++.  Test infrastructure only: the product never builds this.
#include "../../vamp_amd/csrc/metric_host.hpp"

#include <iostream>
#include <limits>

using namespace vamp::metric;

namespace {

int failures = 0;

void expect(bool ok, const std::string& what) {
    if (!ok) {
        std::cout << "FAILED: " << what << "\n";
        ++failures;
    }
}

struct Args {                      // G groups that share one small matrix and its scales: the checks read scales only
    int G;
    std::vector<double> m, s;
    std::vector<const double*> mat, scale;
    std::vector<int64_t> ld;
    std::vector<int32_t> dim, n_mat, kind;
    std::vector<double> lo, hi;
    int n_sweeps = 8, is_device = 0, out_is_device = 0;

    explicit Args(int G_, int D = 3) : G(G_), m((size_t)D * D, 1.0), s((size_t)D, 2.0), mat(G_, m.data()), scale(G_, s.data()), ld(G_, D), dim(G_, D),
                                      n_mat(G_, 1), kind(G_, 0), lo(G_, 1.0), hi(G_, 4.0) {}

    std::string run(Layout& L) const {
        return check_args("fn: ", G, mat.data(), is_device, ld.data(), dim.data(), n_mat.data(), scale.data(), kind.data(), lo.data(), hi.data(),
                          n_sweeps, out_is_device, L);
    }
    std::string run() const {
        Layout L;
        return run(L);
    }
};

bool has(const std::string& msg, const std::string& part) { return msg.find(part) != std::string::npos; }

}  // namespace

int main() {
    // the plan: as many matrices per workgroup as fit, one at least, the stride odd
    for (int D = 1; D <= kMaxDim; ++D) {
        const Plan p = plan(D);
        std::cout << "plan " << D << " " << p.waves << " " << p.lds << "\n";
        expect(p.waves >= 1 && p.waves <= kMaxWaves, "waves in range");
        expect(p.lds <= kLdsBudget && p.lds == sizeof(double) * (size_t)p.waves * slot_doubles(D), "lds is waves slots, inside the budget");
        expect(p.waves == kMaxWaves || sizeof(double) * (size_t)(p.waves + 1) * slot_doubles(D) > kLdsBudget, "one more matrix would not fit");
        expect(row_stride(D) % 2 == 1 && row_stride(D) > padded(D) && padded(D) >= D && padded(D) % 2 == 0 && padded(D) - D <= 1, "padding and stride");
    }
    expect(plan(kMaxDim).waves == 2 && plan(48).waves == 4 && sizeof(double) * slot_doubles(kMaxDim) > 64 * 1024, "the largest D needs the raised limit");

    // a good call and its layout
    {
        Args a(3);
        a.dim = {3, 3, 3};
        a.n_mat = {2, 1, 5};
        a.ld = {3, 7, 4};
        Layout L;
        expect(a.run(L).empty(), "good arguments pass");
        expect(L.tot_pt == 8 && L.tot_vec == 24 && L.tot_mat == 72 && L.tot_scale == 9 && L.max_dim == 3, "totals");
        expect(L.o_pt[2] == 3 && L.o_vec[2] == 9 && L.o_mat[1] == 18 && L.o_scale[1] == 3, "offsets");
        expect(L.span[0] == 5 * 3 + 3 && L.span[1] == 2 * 7 + 3 && L.span[2] == 14 * 4 + 3 && L.tot_span == 18 + 17 + 59, "host spans");
        a.is_device = 1;
        expect(a.run(L).empty() && L.tot_span == 0, "no host span for device matrices");
    }
    // every refusal
    {
        Args a(1);
        a.G = 0;
        expect(has(a.run(), "n_groups"), "n_groups");
    }
    {
        Args a(1);
        Layout L;
        expect(has(check_args("fn: ", 1, nullptr, 0, a.ld.data(), a.dim.data(), a.n_mat.data(), a.scale.data(), a.kind.data(), a.lo.data(), a.hi.data(), 8, 0, L),
                   "NULL argument"), "NULL list");
        a.mat[0] = nullptr;
        expect(has(a.run(), "NULL matrix or scale"), "NULL matrix");
    }
    for (int bad : {0, kMaxSweeps + 1, -1}) {
        Args a(1);
        a.n_sweeps = bad;
        expect(has(a.run(), "n_sweeps"), "n_sweeps");
    }
    for (int bad : {0, kMaxDim + 1, -5, std::numeric_limits<int32_t>::max()}) {
        Args a(2);
        a.dim[1] = bad;
        expect(has(a.run(), "group 1: dim"), "dim");
    }
    {
        Args a(1);
        a.n_mat[0] = 0;
        expect(has(a.run(), "n_mat"), "n_mat");
        a.n_mat[0] = 1;
        a.ld[0] = 2;
        expect(has(a.run(), "ld = 2"), "ld below D");
        a.ld[0] = 3;
        a.kind[0] = 2;
        expect(has(a.run(), "kind"), "kind");
        a.kind[0] = 1;
        a.is_device = 2;
        expect(has(a.run(), "is_device"), "is_device");
        a.is_device = 0;
        a.out_is_device = -1;
        expect(has(a.run(), "out_is_device"), "out_is_device");
    }
    for (double bad : {0.0, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
        Args a(1);
        a.s[2] = bad;
        expect(has(a.run(), "entry 2"), "scale");
        Args b(1);
        b.lo[0] = bad;
        b.hi[0] = std::numeric_limits<double>::infinity();
        expect(has(b.run(), "lam_lo"), "lam_lo");
    }
    {
        Args a(1);
        a.hi[0] = 0.5;
        expect(has(a.run(), "lam_hi"), "lam_hi below lam_lo");
        a.hi[0] = std::numeric_limits<double>::quiet_NaN();
        expect(has(a.run(), "lam_hi"), "lam_hi NaN");
        a.hi[0] = std::numeric_limits<double>::infinity();
        expect(a.run().empty(), "lam_hi = +inf is allowed");
        a.hi[0] = a.lo[0];
        expect(a.run().empty(), "lam_hi = lam_lo is allowed");
    }
    // the limits, where sums could overflow
    {
        Args a(1, kMaxDim);
        a.n_mat[0] = std::numeric_limits<int32_t>::max();
        a.ld[0] = std::numeric_limits<int64_t>::max();
        expect(has(a.run(), "matrix entries"), "n_mat at its largest");
        a.n_mat[0] = 1;
        expect(has(a.run(), "ld is beyond"), "ld at its largest");
        a.ld[0] = kMaxMatrixDoubles;
        a.n_mat[0] = (int32_t)(kMaxMatrixDoubles / (kMaxDim * kMaxDim));
        expect(has(a.run(), "to copy from host memory"), "the host span at its largest");
        a.is_device = 1;
        Layout L;
        expect(a.run(L).empty() && L.tot_mat <= kMaxMatrixDoubles && L.span[0] > 0, "the same from device memory");
        a.n_mat[0] += 1;
        expect(has(a.run(), "matrix entries"), "one matrix past the bound");
    }
    {
        Args a(4, kMaxDim);                                     // the bound is on the sum over the groups
        for (int g = 0; g < 4; ++g) a.n_mat[g] = (int32_t)(kMaxMatrixDoubles / (kMaxDim * kMaxDim) / 4);
        a.is_device = 1;
        expect(a.run().empty(), "four groups inside the bound");
        a.n_mat[3] += 4;
        expect(has(a.run(), "matrix entries"), "four groups past it");
    }
    if (failures) return 1;
    std::cout << "checks ok\n";
    return 0;
}
