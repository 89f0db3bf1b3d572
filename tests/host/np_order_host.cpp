// Host build of vamp::np_pair_order (vamp_amd/csrc/ff_predicates.hpp) for tests/test_node_pass_order.py: the order in
// which the node pass of a full batch takes the batch's far lines.  Test infrastructure only: the product never loads this.
#include "../../vamp_amd/csrc/ff_predicates.hpp"
#include <cstdint>

extern "C" void np_pair_order_host(int64_t n, const uint32_t* far, const uint32_t* n6, const uint32_t* n4, const uint32_t* n3, uint64_t* seq,
                                   uint32_t* solo, int32_t* pairs) {
    for (int64_t i = 0; i < n; ++i) {
        const vamp::NpOrder o = vamp::np_pair_order(far[i], n6[i], n4[i], n3[i]);
        seq[i] = o.seq;
        solo[i] = o.solo;
        for (int d = 0; d < 4; ++d) pairs[4 * i + d] = o.pairs[d];
    }
}
