// chain_groups.hpp -- what the libraries that walk every sample of every group's chain over the group's pixels
// (posterior.hip, predictive.hip, loo.hip) share on the host: the checks of the per-group chain arguments, and the plan
// that cuts the [S samples] x [P pixels] scratch matrices of all groups into passes; for the two that evaluate a
// log-likelihood (predictive.hip, loo.hip) also the checks and the packing of the data.  DESIGN.md "The call frame of
// the side libraries".
//
// Host code only, and no HIP: tests/host/chain_groups_host.cpp builds it with plain g++.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace vamp {
namespace side {

constexpr long long kDefaultScratch = 256ll << 20;     // bytes, for scratch_bytes = 0

struct ChainGroups {
    std::vector<int> S, D;         // per group: samples n_keep * walkers, parameters per sample
    int s_max = 0;                 // largest S
    long long tot_pix = 0, tot_s = 0;
    long long cap = 0;             // doubles of scratch a pass may use; cap >= s_max
};

// The checks of n_groups > 0 groups (arrays not NULL: the entry point has seen to both) that do not depend on what
// the library computes; fills `cg`.  Returns "" or the message for *_last_error: `fn` ("name: ") opens it, `hint`
// closes the one about too many samples.
inline std::string check_chain_groups(const std::string& fn, int n_groups, const double* const* x, const int32_t* n_pix,
                                      const int32_t* n_comp, const int32_t* mode, const int32_t* sample_sd, const double* const* base,
                                      const int64_t* ld, const int32_t* n_keep, const int32_t* walkers, int64_t scratch_bytes,
                                      int max_samples, int max_components, const char* hint, ChainGroups& cg) {
    if (scratch_bytes < 0) return fn + "scratch_bytes must not be negative";
    cg = ChainGroups{};
    cg.S.resize(n_groups);
    cg.D.resize(n_groups);
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (!base[g]) return at + "NULL base pointer";
        if (!x[g]) return at + "NULL abscissa";
        if (n_pix[g] <= 0) return at + "n_pix must be positive";
        if (n_comp[g] < 1 || n_comp[g] > max_components)
            return at + "n_comp = " + std::to_string(n_comp[g]) + " is outside 1 .. " + std::to_string(max_components);
        if (mode[g] == 2) return at + "mode 2 (NBZ3) is not supported: pass the chain in the GAUSS3 (0) or VOIGT4 (1) layout";
        if (mode[g] != 0 && mode[g] != 1) return at + "mode must be 0 (GAUSS3) or 1 (VOIGT4)";
        if (sample_sd[g] != 0 && sample_sd[g] != 1) return at + "sample_sd must be 0 or 1";
        if (n_keep[g] <= 0 || walkers[g] <= 0) return at + "n_keep and walkers must be positive";
        const long long S = (long long)n_keep[g] * walkers[g];
        if (S > max_samples)
            return at + "n_keep * walkers = " + std::to_string(S) + " exceeds " + std::to_string(max_samples) + " (" + hint + ")";
        cg.D[g] = (mode[g] == 1 ? 4 : 3) * n_comp[g] + sample_sd[g];
        if (ld[g] < (int64_t)walkers[g] * cg.D[g]) return at + "ld < walkers * ndim";
        for (int p = 0; p < n_pix[g]; ++p)
            if (!std::isfinite(x[g][p])) return at + "the abscissa is not finite at pixel " + std::to_string(p);
        cg.S[g] = (int)S;
        cg.s_max = cg.S[g] > cg.s_max ? cg.S[g] : cg.s_max;
        cg.tot_pix += n_pix[g];
        cg.tot_s += S;
    }
    cg.cap = (scratch_bytes ? scratch_bytes : kDefaultScratch) / (long long)sizeof(double);
    if (cg.cap < cg.s_max)
        return fn + "scratch_bytes = " + std::to_string(scratch_bytes) + " is less than one column of the largest group (" +
               std::to_string((long long)cg.s_max * (long long)sizeof(double)) + " bytes)";
    return "";
}

// The checks of the data a log-likelihood is evaluated against (predictive.hip, loo.hip), after check_chain_groups has
// passed: a flux per group, a noise exactly where the chain does not sample its sd, finite flux, finite positive noise.
// Returns "" or the message; tot_noise: the pixels of the groups with known noise.
inline std::string check_chain_data(const std::string& fn, int n_groups, const double* const* flux, const double* const* noise,
                                    const int32_t* n_pix, const int32_t* sample_sd, long long& tot_noise) {
    tot_noise = 0;
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (!flux[g]) return at + "NULL flux";
        if (sample_sd[g] && noise[g]) return at + "noise must be NULL when sample_sd is set: the chain's sd is the noise";
        if (!sample_sd[g] && !noise[g]) return at + "NULL noise without sample_sd";
        for (int p = 0; p < n_pix[g]; ++p) {
            if (!std::isfinite(flux[g][p])) return at + "the flux is not finite at pixel " + std::to_string(p);
            if (noise[g] && !(std::isfinite(noise[g][p]) && noise[g][p] > 0.0))
                return at + "the noise is not finite and positive at pixel " + std::to_string(p);
        }
        tot_noise += noise[g] ? n_pix[g] : 0;
    }
    return "";
}

struct DataOffsets {               // of one vector of doubles: abscissae | data | noise | ln noise
    long long x = 0, y = 0, noise = 0, ln_noise = 0, end = 0;
};

// The data of all groups in one vector for one upload, laid out as `off`: a group's pixels side by side in group
// order; the noise sections hold only the groups with known noise (noise[g] not NULL).
inline std::vector<double> pack_chain_data(int n_groups, const double* const* x, const double* const* flux, const double* const* noise,
                                           const int32_t* n_pix, long long tot_pix, long long tot_noise, DataOffsets& off) {
    off.x = 0;
    off.y = off.x + tot_pix;
    off.noise = off.y + tot_pix;
    off.ln_noise = off.noise + tot_noise;
    off.end = off.ln_noise + tot_noise;
    std::vector<double> h((size_t)off.end);
    long long op = 0, on = 0;
    for (int g = 0; g < n_groups; ++g) {
        for (int p = 0; p < n_pix[g]; ++p) {
            h[off.x + op + p] = x[g][p];
            h[off.y + op + p] = flux[g][p];
            if (noise[g]) {
                h[off.noise + on + p] = noise[g][p];
                h[off.ln_noise + on + p] = std::log(noise[g][p]);
            }
        }
        op += n_pix[g];
        on += noise[g] ? n_pix[g] : 0;
    }
    return h;
}

struct Range {                     // pixels p0 .. p0 + np - 1 of a group: an [S] x [np] matrix of the scratch
    int group, p0, np;
    long long offset;              // of the matrix in its pass's scratch, in doubles
    int pass;
};

struct PassPlan {
    std::vector<Range> ranges;     // in group order, a group's in pixel order
    std::vector<size_t> first;     // per pass: its first range (the one at offset 0)
    long long scratch_len = 0;     // doubles the largest pass uses
};

// Greedy packing in group order: a range takes as many of its group's remaining columns (S doubles each) as fit what
// is left of the pass's cap doubles; when not even one fits, the pass is closed and the next begins empty.  So a
// group is split only at a pass boundary, no pass is empty, and no pass holds two ranges of one group.  cap must be
// at least the largest S (check_chain_groups): otherwise the plan ends before the group that does not fit.
inline PassPlan plan_passes(long long cap, const std::vector<int>& S, const int32_t* n_pix, int G) {
    PassPlan pl;
    long long used = 0;
    for (int g = 0; g < G; ++g)
        for (int p0 = 0; p0 < n_pix[g];) {
            const long long fit = (cap - used) / S[g];
            if (fit == 0) {
                if (used == 0) return pl;
                used = 0;
                continue;
            }
            if (used == 0) pl.first.push_back(pl.ranges.size());
            const int np = (int)((long long)(n_pix[g] - p0) < fit ? (n_pix[g] - p0) : fit);
            pl.ranges.push_back(Range{g, p0, np, used, (int)pl.first.size() - 1});
            used += (long long)np * S[g];
            pl.scratch_len = used > pl.scratch_len ? used : pl.scratch_len;
            p0 += np;
        }
    return pl;
}

}  // namespace side
}  // namespace vamp
