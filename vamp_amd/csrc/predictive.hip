// predictive.hip -- pointwise log predictive density and WAIC of ensemble chains
// (include/vamp_pred.h, libvamp_pred.so).  Definitions: DESIGN.md "Pointwise predictive density and WAIC".
//
// The work is a list of items (group, pixel range), packed greedily into passes whose log-likelihood scratch fits
// scratch_bytes (chain_groups.hpp, which posterior.hip and loo.hip share).  Two launches per pass, one at the end:
//   k_pointwise_ll the evaluation this library shares with loo.hip (pointwise_ll.hpp): one workgroup per (item, 64
//                  samples) writes the log-likelihood of every pixel's datum, l_sp, to the scratch matrix.
//   k_pred_column  one workgroup of 1024 threads per column (a pixel's l over the samples).  A thread holds its at
//                  most 16 entries in registers; the maximum, the sum of exponentials, the sum and the centred sum of
//                  squares are each a per-thread fold in sample order and a block reduction of fixed order, so a
//                  column's result does not depend on the pass it was packed into.
//   k_pred_totals  one thread per group: the group's sums over its per-pixel values, in pixel order.
// No kernel asks for more than 64 KiB of LDS: the evaluation's largest launch (32 lines, four wavefronts) takes
// 51 200 bytes, the column stage 8 KiB.  Everything is fp64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_pred.h"
#include "chain_groups.hpp"
#include "lane_group.hpp"
#include "pointwise_ll.hpp"
#include "side_call.hpp"
#include "voigt_math.hpp"

#define VAMP_PRED_API extern "C" __attribute__((visibility("default")))

// Orientation of the scratch of an item ([S samples] x [np pixels]):
//   0  sample-major, ll[s * np + p]: the evaluation's stores are contiguous, the column loads strided
//   1  pixel-major,  ll[p * S + s]: the column loads are contiguous, the evaluation's stores strided
// and whether a 16-lane group may own a sample.  Neither changes a bit of a result; both are decided by measurement
// (profiles/predictive_bench.txt, q1422 shape, ms per call, alternating builds in one process): pixel-major 14.1 against
// sample-major 15.7 -- the column stage is three light passes over a column, so its loads decide, unlike the sort of
// k_post_column; 16-lane groups 14.2 against 16.5 without -- used.
#ifndef VAMP_PRED_PIXEL_MAJOR
#define VAMP_PRED_PIXEL_MAJOR 1
#endif
#ifndef VAMP_PRED_NARROW
#define VAMP_PRED_NARROW 1
#endif

namespace {

using namespace vamp::side;

constexpr int kColBlock = 1024;            // one size for every column: the reduction order must not depend on the pass
constexpr int kColPerThread = VAMP_PRED_MAX_SAMPLES / kColBlock;
constexpr int kTotBlock = 64;
constexpr double kHighPwaic = 0.4;         // Vehtari, Gelman & Gabry (2017)

static_assert(kColPerThread * kColBlock == VAMP_PRED_MAX_SAMPLES && kColPerThread <= 32, "a thread's entries are a bit mask");
static_assert(VAMP_PRED_MAX_COMPONENTS <= kEvalMaxComponents, "the evaluation's LDS is sized for kEvalMaxComponents lines");

struct ColSet {                    // the columns of an item
    const double* src;             // l of (column c, sample s) = src[c * stride_c + s * stride_s]
    const uint8_t* bad;
    double* lppd;                  // [c]
    double* ll_mean;               // [c]
    double* pwaic;                 // [c]
    int32_t* counts;               // {n_used, n_bad} of the group (written by column 0), or NULL
    long long stride_c, stride_s;
    int S;
};

struct Totals {                    // a group's per-pixel values and where its sums go
    const double* lppd;
    const double* ll_mean;
    const double* pwaic;
    int P;
};

__global__ __launch_bounds__(kColBlock) void k_pred_column(const ColSet* __restrict__ sets, const int2* __restrict__ tasks) {
    __shared__ double red[kColBlock];
    const int2 task = tasks[blockIdx.x];
    const ColSet C = sets[task.x];
    const int c = task.y, tid = threadIdx.x;
    const double* src = C.src + (long long)c * C.stride_c;

    double v[kColPerThread];
    unsigned have = 0u;                                // the thread's entries that are good samples
    double nb = 0.0, nn = 0.0;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j) {
        const int i = tid + j * kColBlock;
        v[j] = 0.0;
        if (i < C.S) {
            if (C.bad[i]) nb += 1.0;
            else {
                v[j] = src[(long long)i * C.stride_s];
                have |= 1u << j;
                if (isnan(v[j])) nn += 1.0;
            }
        }
    }
    const int n_bad = (int)vamp::block_sum<kColBlock>(nb, red);
    const int n_nan = (int)vamp::block_sum<kColBlock>(nn, red);
    const int n = C.S - n_bad;

    double part = -INFINITY;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j)
        if (have >> j & 1u) part = fmax(part, v[j]);
    const double m = vamp::block_max<kColBlock>(part, red);
    double pe = 0.0, ps = 0.0;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j)
        if (have >> j & 1u) { pe += exp(v[j] - m); ps += v[j]; }
    const double sum_exp = vamp::block_sum<kColBlock>(pe, red);
    const double mean = vamp::block_sum<kColBlock>(ps, red) / (double)n;
    part = 0.0;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j)
        if (have >> j & 1u) { const double d = v[j] - mean; part = fma(d, d, part); }
    const double css = vamp::block_sum<kColBlock>(part, red);

    if (tid == 0) {
        const bool none = n == 0 || n_nan > 0;         // a NaN among the values makes every statistic NaN
        C.lppd[c] = none ? NAN : m + log(sum_exp / (double)n);
        C.ll_mean[c] = none ? NAN : mean;
        C.pwaic[c] = (none || n < 2) ? NAN : css / (double)(n - 1);
        if (C.counts && c == 0) { C.counts[0] = n; C.counts[1] = n_bad; }
    }
}

// out: [4][G] doubles (elpd_waic, elpd_se, p_waic, lnl_mean); n_high: [G]
__global__ __launch_bounds__(kTotBlock) void k_pred_totals(const Totals* __restrict__ tot, int G, double* __restrict__ out,
                                                           int32_t* __restrict__ n_high) {
    const int g = blockIdx.x * kTotBlock + threadIdx.x;
    if (g >= G) return;
    const Totals T = tot[g];
    double elpd = 0.0, pw = 0.0, lm = 0.0;
    int high = 0;
    for (int p = 0; p < T.P; ++p) {
        const double w = T.pwaic[p];
        elpd += T.lppd[p] - w;
        pw += w;
        lm += T.ll_mean[p];
        high += w > kHighPwaic ? 1 : 0;
    }
    const double mean = elpd / (double)T.P;
    double ss = 0.0;
    for (int p = 0; p < T.P; ++p) {
        const double d = (T.lppd[p] - T.pwaic[p]) - mean;
        ss = fma(d, d, ss);
    }
    out[g] = elpd;
    out[G + g] = T.P < 2 ? NAN : sqrt((double)T.P * (ss / (double)(T.P - 1)));
    out[2 * G + g] = pw;
    out[3 * G + g] = lm;
    n_high[g] = high;
}

struct Pass {
    size_t etask0, etask1;         // its k_pointwise_ll workgroups
    size_t ctask0, ctask1;         // its k_pred_column workgroups
    int region_doubles = 0;        // LDS of a wavefront of k_pointwise_ll
};

}  // namespace

VAMP_PRED_API int vamp_pred_version(void) { return VAMP_PRED_ABI_VERSION; }

VAMP_PRED_API const char* vamp_pred_last_error(void) { return g_err.c_str(); }

VAMP_PRED_API int vamp_pred_pointwise(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                                      const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                                      const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                                      const int32_t* n_keep, const int32_t* walkers, int64_t scratch_bytes, double* lppd,
                                      double* ll_mean, double* p_waic_pix, double* elpd_waic, double* elpd_se, double* p_waic,
                                      double* lnl_mean, int32_t* n_high, int32_t* n_used, int32_t* n_bad) {
    g_err.clear();
    const std::string fn = "vamp_pred_pointwise: ";
    if (n_groups <= 0) return fail(fn + "n_groups must be positive");
    if (!x || !flux || !noise || !n_pix || !n_comp || !mode || !sample_sd || !base || !ld || !n_keep || !walkers)
        return fail(fn + "NULL argument");
    ChainGroups cg;
    const std::string err = check_chain_groups(fn, n_groups, x, n_pix, n_comp, mode, sample_sd, base, ld, n_keep, walkers, scratch_bytes,
                                               VAMP_PRED_MAX_SAMPLES, VAMP_PRED_MAX_COMPONENTS,
                                               "subsample in time: ld * step, ceil(n_keep / step)", cg);
    if (!err.empty()) return fail(err);
    const long long tot_pix = cg.tot_pix, tot_s = cg.tot_s;
    long long tot_noise = 0;
    const std::string data_err = check_chain_data(fn, n_groups, flux, noise, n_pix, sample_sd, tot_noise);
    if (!data_err.empty()) return fail(data_err);
    if (tot_pix > (1LL << 30)) return fail(fn + "too many outputs");

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    // device view of every group's chain: staged (host input) or as given
    std::vector<const double*> dbase(base, base + n_groups);
    DevBuf staging;
    if (!is_device) {
        std::vector<long long> len(n_groups);
        for (int g = 0; g < n_groups; ++g) len[g] = chain_span(n_keep[g], ld[g], walkers[g], cg.D[g]);
        if (stage_chains(len, base, st, staging, dbase)) return -1;
    }

    // one buffer of doubles: abscissae | data | noise | ln noise | per-pixel outputs | group outputs
    DataOffsets in;
    const std::vector<double> h_in = pack_chain_data(n_groups, x, flux, noise, n_pix, tot_pix, tot_noise, in);
    const long long o_lppd = in.end, o_lm = o_lppd + tot_pix, o_pw = o_lm + tot_pix, o_grp = o_pw + tot_pix, o_end = o_grp + 4ll * n_groups;
    DevBuf d_main, d_bad, d_counts, d_scratch;
    HIP_TRY(hipMalloc(&d_main.p, (size_t)o_end * sizeof(double)));
    HIP_TRY(hipMalloc(&d_bad.p, (size_t)tot_s));
    HIP_TRY(hipMalloc(&d_counts.p, (size_t)n_groups * 3 * sizeof(int32_t)));     // {n_used, n_bad} per group, then n_high
    HIP_TRY(hipMemcpyAsync(d_main.p, h_in.data(), h_in.size() * sizeof(double), hipMemcpyHostToDevice, st));
    double* dm = d_main.as<double>();

    // the plan (chain_groups.hpp): one item (pointwise_ll.hpp) and one column set per range, a group's totals after
    // its last range
    const PassPlan plan = plan_passes(cg.cap, cg.S, n_pix, n_groups);
    HIP_TRY(hipMalloc(&d_scratch.p, (size_t)plan.scratch_len * sizeof(double)));
    std::vector<Item> items;
    std::vector<ColSet> sets;
    std::vector<Totals> totals;
    std::vector<int2> etasks, ctasks;
    std::vector<Pass> passes(plan.first.size());
    build_eval(plan, cg, in, dm, noise, n_pix, n_comp, mode, ld, walkers, dbase, VAMP_PRED_NARROW != 0, d_scratch.as<double>(),
               d_bad.as<uint8_t>(), items, etasks, passes);
    long long pix_off = 0, s_off = 0;                    // of the range's group
    for (const Range& r : plan.ranges) {
        const int g = r.group, S = cg.S[g], P = n_pix[g], p0 = r.p0, np = r.np;
        Pass& ps = passes[r.pass];
        if (r.offset == 0) ps.ctask0 = ctasks.size();
        ColSet cs;
        cs.src = d_scratch.as<double>() + r.offset;
        cs.bad = d_bad.as<uint8_t>() + s_off;
        cs.lppd = dm + o_lppd + pix_off + p0;
        cs.ll_mean = dm + o_lm + pix_off + p0;
        cs.pwaic = dm + o_pw + pix_off + p0;
        cs.counts = p0 == 0 ? d_counts.as<int32_t>() + 2 * g : nullptr;
        cs.stride_c = VAMP_PRED_PIXEL_MAJOR ? S : 1;
        cs.stride_s = VAMP_PRED_PIXEL_MAJOR ? 1 : np;
        cs.S = S;
        const int ii = (int)sets.size();
        sets.push_back(cs);
        for (int c = 0; c < np; ++c) ctasks.push_back(make_int2(ii, c));
        ps.ctask1 = ctasks.size();
        if (p0 + np == P) {
            Totals t;
            t.lppd = dm + o_lppd + pix_off; t.ll_mean = dm + o_lm + pix_off; t.pwaic = dm + o_pw + pix_off; t.P = P;
            totals.push_back(t);
            pix_off += P; s_off += S;
        }
    }
    if (etasks.size() > 0x7fffffff || ctasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");

    DevBuf d_items, d_sets, d_totals, d_etasks, d_ctasks;
    if (upload(d_items, items, st) || upload(d_sets, sets, st) || upload(d_totals, totals, st) || upload(d_etasks, etasks, st) ||
        upload(d_ctasks, ctasks, st))
        return -1;
    for (const Pass& ps : passes) {
        if (launch_eval<VAMP_PRED_PIXEL_MAJOR != 0>(ps, d_items, d_etasks, st)) return -1;
        hipLaunchKernelGGL(k_pred_column, dim3((unsigned)(ps.ctask1 - ps.ctask0)), dim3(kColBlock), 0, st, d_sets.as<ColSet>(),
                           d_ctasks.as<int2>() + ps.ctask0);
        HIP_TRY(hipGetLastError());
    }
    int32_t* d_high = d_counts.as<int32_t>() + 2 * n_groups;
    hipLaunchKernelGGL(k_pred_totals, dim3((unsigned)((n_groups + kTotBlock - 1) / kTotBlock)), dim3(kTotBlock), 0, st,
                       d_totals.as<Totals>(), n_groups, dm + o_grp, d_high);
    HIP_TRY(hipGetLastError());

    const long long sz = sizeof(double), G = n_groups;
    if (fetch(lppd, dm + o_lppd, tot_pix * sz, st) || fetch(ll_mean, dm + o_lm, tot_pix * sz, st) ||
        fetch(p_waic_pix, dm + o_pw, tot_pix * sz, st) || fetch(elpd_waic, dm + o_grp, G * sz, st) ||
        fetch(elpd_se, dm + o_grp + G, G * sz, st) || fetch(p_waic, dm + o_grp + 2 * G, G * sz, st) ||
        fetch(lnl_mean, dm + o_grp + 3 * G, G * sz, st) || fetch(n_high, d_high, G * (long long)sizeof(int32_t), st))
        return -1;
    return fetch_counts(d_counts, n_groups, n_used, n_bad, st);
}
