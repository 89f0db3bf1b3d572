// relabel_host.hpp -- what relabel.hip does on the host before its first HIP call: the checks of the per-group
// arguments of vamp_relabel_chains and of vamp_relabel_assign, the width of the lane group that owns a sample, and the
// layout of the per-sample, per-column and per-chunk device arrays of all groups.  DESIGN.md "Relabelling: undoing
// label switching".
//
// Host code only, and no HIP: tests/host/relabel_host.cpp builds it with plain g++.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace vamp {
namespace relabel {

constexpr int kMaxComponents = 32;     // VAMP_RELABEL_MAX_COMPONENTS
constexpr int kChunk = 64;             // samples of one partial sum of the moments: fixed, so that no sum depends on the packing

// lanes of the group that owns one sample: from K alone (lane j owns reference line j)
constexpr int group_lanes(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : 32; }

constexpr long long n_chunks(long long S) { return (S + kChunk - 1) / kChunk; }

struct Groups {
    std::vector<int> S, D, q, lanes;           // per group: samples, parameters per sample, per line, lanes per sample
    std::vector<long long> samp_off;           // of the group's first sample in the per-sample arrays (cost, flags)
    std::vector<long long> perm_off;           // of its first byte in the permutations: samp_off scaled by K, summed
    std::vector<long long> part_off;           // of its first double in the partial sums: [chunk][q K]
    std::vector<int> col_off, sc_off;          // of its first column (q K per group) and its first scale (q per group)
    long long tot_s = 0, tot_perm = 0, tot_part = 0;
    int tot_col = 0, tot_sc = 0;
};

// the doubles from the first sample of a chain to the end of its last
inline long long span(int n_keep, long long ld, int walkers, int ndim) {
    return (long long)(n_keep - 1) * ld + (long long)walkers * ndim;
}

// The checks of vamp_relabel_chains (n_groups > 0 and the arrays not NULL: the entry point has seen to both); fills
// `rg`.  Returns "" or the message for vamp_relabel_last_error; `fn` ("name: ") opens it.
inline std::string check_groups(const std::string& fn, int n_groups, const int32_t* n_comp, const int32_t* mode,
                                const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                                const int32_t* n_keep, const int32_t* walkers, const double* const* ref, const double* const* scale,
                                int max_iter, double* const* out, const int64_t* out_ld, int out_is_device, Groups& rg) {
    if (max_iter < 1) return fn + "max_iter must be at least 1";
    if (out && !out_ld) return fn + "out without out_ld";
    rg = Groups{};
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (!base[g]) return at + "NULL base pointer";
        if (n_comp[g] < 1 || n_comp[g] > kMaxComponents)
            return at + "n_comp = " + std::to_string(n_comp[g]) + " is outside 1 .. " + std::to_string(kMaxComponents);
        if (mode[g] == 2) return at + "mode 2 (NBZ3) is not supported: pass the chain in the GAUSS3 (0) or VOIGT4 (1) layout";
        if (mode[g] != 0 && mode[g] != 1) return at + "mode must be 0 (GAUSS3) or 1 (VOIGT4)";
        if (sample_sd[g] != 0 && sample_sd[g] != 1) return at + "sample_sd must be 0 or 1";
        if (n_keep[g] <= 0 || walkers[g] <= 0) return at + "n_keep and walkers must be positive";
        const long long S = (long long)n_keep[g] * walkers[g];
        if (S >= (1ll << 31)) return at + "n_keep * walkers = " + std::to_string(S) + " is not below 2^31";
        const int K = n_comp[g], q = mode[g] == 1 ? 4 : 3, D = q * K + sample_sd[g];
        if (ld[g] < (int64_t)walkers[g] * D) return at + "ld < walkers * ndim";
        if (!ref[g]) return at + "NULL ref";
        for (int e = 0; e < K * q; ++e)
            if (!std::isfinite(ref[g][e]))
                return at + "ref is not finite at line " + std::to_string(e / q) + ", parameter " + std::to_string(e % q);
        if (scale && scale[g])
            for (int d = 0; d < q; ++d)
                if (!(std::isfinite(scale[g][d]) && scale[g][d] > 0.0))
                    return at + "scale is not finite and positive at parameter " + std::to_string(d);
        if (out && out[g]) {
            if (out_ld[g] < (int64_t)walkers[g] * D) return at + "out_ld < walkers * ndim";
            const bool same = out[g] == base[g] && out_ld[g] == ld[g] && !out_is_device == !is_device;
            if (!same && !out_is_device == !is_device) {
                // two ranges of one address space: the rows interleave when they start inside each other, so any
                // overlap of the spans is refused
                const char* a0 = reinterpret_cast<const char*>(base[g]);
                const char* b0 = reinterpret_cast<const char*>(out[g]);
                const char* a1 = a0 + span(n_keep[g], ld[g], walkers[g], D) * (long long)sizeof(double);
                const char* b1 = b0 + span(n_keep[g], out_ld[g], walkers[g], D) * (long long)sizeof(double);
                if (a0 < b1 && b0 < a1)
                    return at + "out overlaps base without being the same chain (in place: out = base and out_ld = ld)";
            }
        }
        rg.S.push_back((int)S);
        rg.D.push_back(D);
        rg.q.push_back(q);
        rg.lanes.push_back(group_lanes(K));
        rg.samp_off.push_back(rg.tot_s);
        rg.perm_off.push_back(rg.tot_perm);
        rg.part_off.push_back(rg.tot_part);
        rg.col_off.push_back(rg.tot_col);
        rg.sc_off.push_back(rg.tot_sc);
        rg.tot_s += S;
        rg.tot_perm += S * K;
        rg.tot_part += n_chunks(S) * (q * K);
        rg.tot_col += q * K;
        rg.tot_sc += q;
    }
    return "";
}

// the checks of vamp_relabel_assign
inline std::string check_assign(const std::string& fn, int K, int n, const double* cost) {
    if (K < 1 || K > kMaxComponents) return fn + "K = " + std::to_string(K) + " is outside 1 .. " + std::to_string(kMaxComponents);
    if (n < 1) return fn + "n must be positive";
    if ((long long)n * K * K >= (1ll << 31)) return fn + "n K K is not below 2^31";
    if (!cost) return fn + "NULL cost";
    return "";
}

// Workgroups of a launch over (group, first unit): `per_block[g]` units (samples, chunks) of group g per workgroup.
// Returns the pairs in group order; the kernels take them as int2.
struct Task { int group, first; };
inline std::vector<Task> plan_tasks(const std::vector<long long>& units, const std::vector<int>& per_block) {
    std::vector<Task> tasks;
    for (size_t g = 0; g < units.size(); ++g)
        for (long long u = 0; u < units[g]; u += per_block[g]) tasks.push_back(Task{(int)g, (int)u});
    return tasks;
}

}  // namespace relabel
}  // namespace vamp
