// Stand-alone host program for tests/test_relabel.py: the checks and the layout of vamp_amd/csrc/relabel_host.hpp as
// relabel.hip compiles them.  Every line of standard input is one case:
//   lanes K                      -> "lanes w"
//   tasks per_block G  u_0 ... u_{G-1}
//                                -> "tasks n | group first | ..."  (per_block units of every group per workgroup)
//   assign K n null              -> "ok" or "error <message>"
//   check max_iter G  then per group: n_comp mode sample_sd n_keep walkers ld  ref(0 ok, 1 NULL, 2 a NaN at its last
//         value)  scale(0 NULL, 1 ok, 2 a zero at its last value)  out(0 none, 1 in place, 2 apart, 3 overlapping, 4 same
//         start but another ld)
//                                -> "ok tot_s tot_perm tot_part tot_col tot_sc | S D q lanes samp_off perm_off part_off col_off sc_off | ..."
//                                   or "error <message>"
// Built with -fsanitize=address,undefined by plain g++.  Test infrastructure only: the product never builds this.
#include "../../vamp_amd/csrc/relabel_host.hpp"

#include <iostream>
#include <limits>
#include <sstream>

int main() {
    using namespace vamp::relabel;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "lanes") {
            int K;
            in >> K;
            std::cout << "lanes " << group_lanes(K) << "\n";
        } else if (what == "tasks") {
            int per, G;
            in >> per >> G;
            std::vector<long long> units(G);
            for (int g = 0; g < G; ++g) in >> units[g];
            const std::vector<Task> tasks = plan_tasks(units, std::vector<int>(G, per));
            std::cout << "tasks " << tasks.size();
            for (const Task& t : tasks) std::cout << " | " << t.group << " " << t.first;
            std::cout << "\n";
        } else if (what == "assign") {
            int K, n, null;
            in >> K >> n >> null;
            const double one = 1.0;
            const std::string err = check_assign("fn: ", K, n, null ? nullptr : &one);
            std::cout << (err.empty() ? "ok" : "error " + err) << "\n";
        } else {
            int max_iter, G;
            in >> max_iter >> G;
            std::vector<int32_t> n_comp(G), mode(G), sd(G), n_keep(G), walkers(G);
            std::vector<int64_t> ld(G), out_ld(G);
            std::vector<std::vector<double>> refs(G), scales(G);
            std::vector<const double*> base(G), ref(G), scale(G);
            std::vector<double*> out(G);
            // addresses only: the checks never read a chain, so one small array stands for all of them
            static double arena[4096];
            bool any_out = false;
            for (int g = 0; g < G; ++g) {
                int ref_kind, scale_kind, out_kind;
                in >> n_comp[g] >> mode[g] >> sd[g] >> n_keep[g] >> walkers[g] >> ld[g] >> ref_kind >> scale_kind >> out_kind;
                const int q = mode[g] == 1 ? 4 : 3, K = n_comp[g] > 0 && n_comp[g] <= 64 ? n_comp[g] : 1;
                refs[g].assign((size_t)K * q, 1.5);
                if (ref_kind == 2) refs[g].back() = std::numeric_limits<double>::quiet_NaN();
                ref[g] = ref_kind == 1 ? nullptr : refs[g].data();
                scales[g].assign(q, 2.0);
                if (scale_kind == 2) scales[g].back() = 0.0;
                scale[g] = scale_kind == 0 ? nullptr : scales[g].data();
                base[g] = arena;
                out_ld[g] = out_kind == 4 ? ld[g] + 1 : ld[g];
                out[g] = out_kind == 0 ? nullptr : (out_kind == 1 || out_kind == 4) ? arena : out_kind == 2 ? arena + 2048 : arena + 1;
                any_out |= out_kind != 0;
            }
            Groups rg;
            const std::string err = check_groups("fn: ", G, n_comp.data(), mode.data(), sd.data(), base.data(), 0, ld.data(), n_keep.data(),
                                                 walkers.data(), ref.data(), scale.data(), max_iter, any_out ? out.data() : nullptr,
                                                 out_ld.data(), 0, rg);
            if (!err.empty()) {
                std::cout << "error " << err << "\n";
                continue;
            }
            std::cout << "ok " << rg.tot_s << " " << rg.tot_perm << " " << rg.tot_part << " " << rg.tot_col << " " << rg.tot_sc;
            for (int g = 0; g < G; ++g)
                std::cout << " | " << rg.S[g] << " " << rg.D[g] << " " << rg.q[g] << " " << rg.lanes[g] << " " << rg.samp_off[g] << " "
                          << rg.perm_off[g] << " " << rg.part_off[g] << " " << rg.col_off[g] << " " << rg.sc_off[g];
            std::cout << "\n";
        }
    }
    return 0;
}
