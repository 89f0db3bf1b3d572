// metric_host.hpp -- what metric.hip does on the host before its first HIP call: the checks of the arguments of
// vamp_metric_factor, the layout of the outputs of all groups, and the plan of a launch (how many matrices share a
// workgroup, and its dynamic LDS).  DESIGN.md section 18.
//
// Host code only, and no HIP: tests/host/metric_host.cpp builds it with plain g++.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace vamp {
namespace metric {

constexpr int kMaxDim = 65;                                // VAMP_METRIC_MAX_DIM
constexpr int kMaxSweeps = 32;                             // VAMP_METRIC_MAX_SWEEPS
constexpr long long kMaxMatrixDoubles = 1LL << 27;         // VAMP_METRIC_MAX_MATRIX_DOUBLES
constexpr int kMaxWaves = 4;                               // matrices of a workgroup: one wavefront each
constexpr size_t kLdsBudget = 160 * 1024 - 1024;           // of a CU's 160 KiB

// D rounded up to even: the order of the padded matrix
constexpr int padded(int D) { return (D + 1) & ~1; }
// doubles between two rows of A and V in LDS: odd, so that the 32 lanes of an LDS lane group -- a lane per row, all at one
// column -- fall on 32 different 8-byte banks; a lane per column at one row is consecutive at any stride
constexpr int row_stride(int D) { return padded(D) + 1; }
// doubles of a wavefront's LDS: A and V; (c, s) per pair, the diagonal, the scales, lam~, 1 / lam~ (first the row sums),
// sqrt(cov_aa); the pairs' slots and the sort order (int32: one double's room for two)
constexpr int slot_doubles(int D) { return 2 * padded(D) * row_stride(D) + 7 * padded(D); }

struct Plan {
    int waves = 0;             // matrices of a workgroup
    int slot = 0;              // doubles of a wavefront's LDS
    size_t lds = 0;            // bytes of a workgroup's dynamic LDS
};

// as many of kMaxWaves matrices per workgroup as the call's largest D leaves room for
inline Plan plan(int max_dim) {
    Plan p;
    p.slot = slot_doubles(max_dim);
    for (p.waves = kMaxWaves; p.waves > 1; --p.waves)
        if (sizeof(double) * (size_t)p.waves * p.slot <= kLdsBudget) break;
    p.lds = sizeof(double) * (size_t)p.waves * p.slot;
    return p;
}
static_assert(sizeof(double) * slot_doubles(kMaxDim) <= kLdsBudget, "one matrix of the largest D fits");

struct Layout {
    std::vector<long long> o_vec, o_mat, o_pt, o_scale, span;      // per group: its first matrix in the outputs; its scales; host doubles
    long long tot_vec = 0, tot_mat = 0, tot_pt = 0, tot_scale = 0, tot_span = 0;
    int max_dim = 0;
};

// The checks of vamp_metric_factor; fills `L`.  Returns "" or the message for vamp_metric_last_error; `fn` ("name: ")
// opens it.
inline std::string check_args(const std::string& fn, int n_groups, const double* const* mat, int is_device, const int64_t* ld,
                              const int32_t* dim, const int32_t* n_mat, const double* const* scale, const int32_t* kind,
                              const double* lam_lo, const double* lam_hi, int n_sweeps, int out_is_device, Layout& L) {
    if (n_groups <= 0) return fn + "n_groups must be positive";
    if (!mat || !ld || !dim || !n_mat || !scale || !kind || !lam_lo || !lam_hi) return fn + "NULL argument";
    if (is_device != 0 && is_device != 1) return fn + "is_device must be 0 or 1";
    if (out_is_device != 0 && out_is_device != 1) return fn + "out_is_device must be 0 or 1";
    if (n_sweeps < 1 || n_sweeps > kMaxSweeps)
        return fn + "n_sweeps = " + std::to_string(n_sweeps) + " is outside 1 .. " + std::to_string(kMaxSweeps);
    L = Layout{};
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        const int D = dim[g];
        if (D < 1 || D > kMaxDim) return at + "dim = " + std::to_string(D) + " is outside 1 .. " + std::to_string(kMaxDim);
        if (n_mat[g] < 1) return at + "n_mat must be at least 1";
        if (!mat[g] || !scale[g]) return at + "NULL matrix or scale";
        if (ld[g] < D) return at + "ld = " + std::to_string((long long)ld[g]) + " is below the " + std::to_string(D) + " entries of a row";
        if (kind[g] != 0 && kind[g] != 1) return at + "kind must be 0 (information) or 1 (covariance)";
        for (int d = 0; d < D; ++d)
            if (!(scale[g][d] > 0.0) || !std::isfinite(scale[g][d])) return at + "scale must be positive and finite (entry " + std::to_string(d) + ")";
        if (!(lam_lo[g] > 0.0) || !std::isfinite(lam_lo[g])) return at + "lam_lo must be positive and finite";
        if (!(lam_hi[g] >= lam_lo[g])) return at + "lam_hi must be at least lam_lo";
        L.o_vec.push_back(L.tot_vec);
        L.o_mat.push_back(L.tot_mat);
        L.o_pt.push_back(L.tot_pt);
        L.o_scale.push_back(L.tot_scale);
        const long long rows = (long long)n_mat[g] * D;
        L.tot_vec += rows;
        L.tot_mat += rows * D;
        L.tot_pt += n_mat[g];
        L.tot_scale += D;
        if (L.tot_mat > kMaxMatrixDoubles)
            return fn + "more than " + std::to_string(kMaxMatrixDoubles) + " matrix entries (sum of n_mat D^2): split the call";
        // (rows and ld are both within 2^27 here: the span cannot overflow)
        if (ld[g] > kMaxMatrixDoubles) return at + "ld is beyond " + std::to_string(kMaxMatrixDoubles);
        const long long sp = (rows - 1) * (long long)ld[g] + D;
        L.span.push_back(sp);
        if (!is_device) L.tot_span += sp;
        if (L.tot_span > kMaxMatrixDoubles)
            return fn + "more than " + std::to_string(kMaxMatrixDoubles) + " doubles to copy from host memory (sum of (n_mat D - 1) ld + D): split the call";
        L.max_dim = D > L.max_dim ? D : L.max_dim;
    }
    return "";
}

}  // namespace metric
}  // namespace vamp
