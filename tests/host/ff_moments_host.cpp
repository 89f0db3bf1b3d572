// Stand-alone host program for tests/test_tile_moments.py: the guard of the moment form (vamp_amd/csrc/ff_moments.hpp)
// as the kernels compile it.  First line of output: the layout constants and the guard's constants.  Then, for every
// line "root_c0 root_q0 amax" on standard input (hexadecimal floats), one line "0" or "1" for ff_moments_ok, with "t" or "f"
// appended for ff_moments_try(root_c0, root_q0).  Built with
// -fsanitize=address,undefined -ffp-contract=off.  Test infrastructure only: the product never builds this.
#include "../../vamp_amd/csrc/ff_moments.hpp"
#include <cstdio>
#include <vector>

int main() {
    std::printf("%d %d %d %d %d %d %d %d %a %a %a\n", vamp::FFM_NS, vamp::FFM_NQ, vamp::FFM_QROW, vamp::FFM_S, vamp::FFM_TILE, vamp::FFM_C0,
                vamp::FFM_RC, vamp::FFM_RQ, vamp::FFM_ULPS, vamp::FFM_BOUND, vamp::FFM_RMAX);
    std::vector<char> out, tried;
    double rc, rq, amax;
    while (std::scanf("%la %la %la", &rc, &rq, &amax) == 3) {
        out.push_back(vamp::ff_moments_ok(rc, rq, amax) ? '1' : '0');
        tried.push_back(vamp::ff_moments_try(rc, rq) ? 't' : 'f');
    }
    for (size_t i = 0; i < out.size(); ++i) std::printf("%c%c\n", out[i], tried[i]);
    return 0;
}
