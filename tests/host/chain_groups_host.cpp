// Stand-alone host program for tests/test_chain_groups.py: the chain checks, the pass planner, the data checks and the
// data packing of vamp_amd/csrc/chain_groups.hpp as the posterior, predictive and LOO libraries compile them.  Every
// line of standard input is one case:
//   plan  cap G  S_0 P_0 ... S_{G-1} P_{G-1}
//         -> "plan scratch_len n_passes | first ... | group p0 np offset pass | ..."
//   check scratch_bytes G  then per group: n_pix n_comp mode sample_sd n_keep walkers ld base_null x_null bad_pixel
//         (bad_pixel: the pixel of the abscissa that is +inf, or -1)
//         -> "ok cap s_max tot_pix tot_s | S D | ..."  or  "error <message>"
//   data  scratch_bytes G  then per group: the fields of check, then flux_null noise_given bad_flux flux_value bad_noise
//         noise_value (bad_flux / bad_noise: the pixel that holds flux_value / noise_value -- "inf", "nan", "0", "-1" --
//         or -1): check_chain_groups, then check_chain_data, as an entry point calls them
//         -> "ok tot_noise"  or  "error <message>"
//   pack  0 G  then per group: n_pix noise_given; x = 100 g + p + 0.25, flux = -(100 g + p) - 0.5, noise = 0.5 + (10 g
//         + p) / 64; a group without noise passes NULL
//         -> "pack x y noise ln_noise end size | h_0 h_1 ..." (%.17g)
// with the limits of both libraries (16 384 samples, 32 lines) and the hint "HINT".  Built with
// -fsanitize=address,undefined.  Test infrastructure only: the product never builds this.
#include "../../vamp_amd/csrc/chain_groups.hpp"

#include <cstdio>
#include <cstdlib>
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
        } else if (what == "pack") {
            std::vector<int32_t> n_pix(G);
            std::vector<std::vector<double>> xs(G), fs(G), ns(G);
            std::vector<const double*> x(G), flux(G), noise(G);
            long long tot_pix = 0, tot_noise = 0;
            for (int g = 0; g < G; ++g) {
                int given;
                in >> n_pix[g] >> given;
                for (int p = 0; p < n_pix[g]; ++p) {
                    xs[g].push_back(100.0 * g + p + 0.25);
                    fs[g].push_back(-(100.0 * g + p) - 0.5);
                    if (given) ns[g].push_back(0.5 + (10.0 * g + p) / 64.0);
                }
                x[g] = xs[g].data();
                flux[g] = fs[g].data();
                noise[g] = given ? ns[g].data() : nullptr;
                tot_pix += n_pix[g];
                tot_noise += given ? n_pix[g] : 0;
            }
            DataOffsets off;
            const std::vector<double> h = pack_chain_data(G, x.data(), flux.data(), noise.data(), n_pix.data(), tot_pix, tot_noise, off);
            std::cout << "pack " << off.x << " " << off.y << " " << off.noise << " " << off.ln_noise << " " << off.end << " " << h.size() << " |";
            char buf[40];
            for (double v : h) {
                std::snprintf(buf, sizeof buf, " %.17g", v);
                std::cout << buf;
            }
            std::cout << "\n";
        } else {
            const bool data = what == "data";
            std::vector<int32_t> n_pix(G), n_comp(G), mode(G), sd(G), n_keep(G), walkers(G);
            std::vector<int64_t> ld(G);
            std::vector<std::vector<double>> xs(G), fs(G), ns(G);
            std::vector<const double*> x(G), base(G), flux(G), noise(G);
            const double chain = 0.0;
            for (int g = 0; g < G; ++g) {
                int base_null, x_null, bad_pixel;
                in >> n_pix[g] >> n_comp[g] >> mode[g] >> sd[g] >> n_keep[g] >> walkers[g] >> ld[g] >> base_null >> x_null >> bad_pixel;
                xs[g].assign(n_pix[g] > 0 ? n_pix[g] : 1, 1.5);    // (never empty: an empty vector's data() may be NULL)
                if (bad_pixel >= 0) xs[g][bad_pixel] = std::numeric_limits<double>::infinity();
                x[g] = x_null ? nullptr : xs[g].data();
                base[g] = base_null ? nullptr : &chain;            // (the checks never read a chain)
                if (!data) continue;
                int flux_null, noise_given, bad_flux, bad_noise;
                std::string flux_value, noise_value;
                in >> flux_null >> noise_given >> bad_flux >> flux_value >> bad_noise >> noise_value;
                fs[g].assign(xs[g].size(), 0.75);
                ns[g].assign(xs[g].size(), 0.125);
                if (bad_flux >= 0) fs[g][bad_flux] = std::strtod(flux_value.c_str(), nullptr);
                if (bad_noise >= 0) ns[g][bad_noise] = std::strtod(noise_value.c_str(), nullptr);
                flux[g] = flux_null ? nullptr : fs[g].data();
                noise[g] = noise_given ? ns[g].data() : nullptr;
            }
            ChainGroups cg;
            const std::string err = check_chain_groups("fn: ", G, x.data(), n_pix.data(), n_comp.data(), mode.data(), sd.data(), base.data(),
                                                       ld.data(), n_keep.data(), walkers.data(), a, 16384, 32, "HINT", cg);
            if (!err.empty()) {
                std::cout << "error " << err << "\n";
                continue;
            }
            if (data) {
                long long tot_noise = -1;
                const std::string derr = check_chain_data("fn: ", G, flux.data(), noise.data(), n_pix.data(), sd.data(), tot_noise);
                if (!derr.empty()) std::cout << "error " << derr << "\n";
                else std::cout << "ok " << tot_noise << "\n";
                continue;
            }
            std::cout << "ok " << cg.cap << " " << cg.s_max << " " << cg.tot_pix << " " << cg.tot_s;
            for (int g = 0; g < G; ++g) std::cout << " | " << cg.S[g] << " " << cg.D[g];
            std::cout << "\n";
        }
    }
    return 0;
}
