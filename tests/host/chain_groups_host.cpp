// Stand-alone host program for tests/test_chain_groups.py: the chain checks and the pass planner of
// vamp_amd/csrc/chain_groups.hpp as the posterior and predictive libraries compile them.  Every line of standard input
// is one case:
//   plan  cap G  S_0 P_0 ... S_{G-1} P_{G-1}
//         -> "plan scratch_len n_passes | first ... | group p0 np offset pass | ..."
//   check scratch_bytes G  then per group: n_pix n_comp mode sample_sd n_keep walkers ld base_null x_null bad_pixel
//         (bad_pixel: the pixel of the abscissa that is +inf, or -1)
//         -> "ok cap s_max tot_pix tot_s | S D | ..."  or  "error <message>"
// with the limits of both libraries (16 384 samples, 32 lines) and the hint "HINT".  Built with
// -fsanitize=address,undefined.  Test infrastructure only: the product never builds this.
#include "../../vamp_amd/csrc/chain_groups.hpp"

#include <iostream>
#include <limits>
#include <sstream>

int main() {
    using namespace vamp::side;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        long long a;
        int G;
        if (!(in >> what >> a >> G)) continue;
        if (what == "plan") {
            std::vector<int> S(G);
            std::vector<int32_t> P(G);
            for (int g = 0; g < G; ++g) in >> S[g] >> P[g];
            const PassPlan pl = plan_passes(a, S, P.data(), G);
            std::cout << "plan " << pl.scratch_len << " " << pl.first.size() << " |";
            for (size_t f : pl.first) std::cout << " " << f;
            for (const Range& r : pl.ranges)
                std::cout << " | " << r.group << " " << r.p0 << " " << r.np << " " << r.offset << " " << r.pass;
            std::cout << "\n";
        } else {
            std::vector<int32_t> n_pix(G), n_comp(G), mode(G), sd(G), n_keep(G), walkers(G);
            std::vector<int64_t> ld(G);
            std::vector<std::vector<double>> xs(G);
            std::vector<const double*> x(G), base(G);
            const double chain = 0.0;
            for (int g = 0; g < G; ++g) {
                int base_null, x_null, bad_pixel;
                in >> n_pix[g] >> n_comp[g] >> mode[g] >> sd[g] >> n_keep[g] >> walkers[g] >> ld[g] >> base_null >> x_null >> bad_pixel;
                xs[g].assign(n_pix[g] > 0 ? n_pix[g] : 1, 1.5);    // (never empty: an empty vector's data() may be NULL)
                if (bad_pixel >= 0) xs[g][bad_pixel] = std::numeric_limits<double>::infinity();
                x[g] = x_null ? nullptr : xs[g].data();
                base[g] = base_null ? nullptr : &chain;            // (the checks never read a chain)
            }
            ChainGroups cg;
            const std::string err = check_chain_groups("fn: ", G, x.data(), n_pix.data(), n_comp.data(), mode.data(), sd.data(), base.data(),
                                                       ld.data(), n_keep.data(), walkers.data(), a, 16384, 32, "HINT", cg);
            if (!err.empty()) {
                std::cout << "error " << err << "\n";
                continue;
            }
            std::cout << "ok " << cg.cap << " " << cg.s_max << " " << cg.tot_pix << " " << cg.tot_s;
            for (int g = 0; g < G; ++g) std::cout << " | " << cg.S[g] << " " << cg.D[g];
            std::cout << "\n";
        }
    }
    return 0;
}
