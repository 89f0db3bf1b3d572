// predictive.hip -- pointwise log predictive density and WAIC of ensemble chains
// (include/vamp_pred.h, libvamp_pred.so).  Definitions: DESIGN.md "Pointwise predictive density and WAIC".
//
// The work is a list of items (group, pixel range), packed greedily into passes whose log-likelihood scratch fits
// scratch_bytes, as posterior.hip packs its flux scratch.  Two launches per pass, one at the end:
//   k_pred_eval    one workgroup per (item, 64 samples).  A wavefront -- or, for short regions of few lines, a
//                  16-lane group -- owns a sample: its parameters become line records and near-axis tables in LDS
//                  once (lane_group.hpp), then its lanes walk the item's pixels and write the log-likelihood of the
//                  pixel's datum, l_sp, to the scratch matrix.
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
#include "lane_group.hpp"
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
using vamp::lds_fence;

constexpr int kEvalBlock = 256;            // four wavefronts
constexpr int kEvalWaves = kEvalBlock / 64;
constexpr int kSamplesPerBlock = 64;
constexpr int kRec = 6;                    // doubles of a line record
constexpr int kColBlock = 1024;            // one size for every column: the reduction order must not depend on the pass
constexpr int kColPerThread = VAMP_PRED_MAX_SAMPLES / kColBlock;
constexpr int kTotBlock = 64;
constexpr long long kDefaultScratch = 256ll << 20;
constexpr double SQRT_LN2 = 0.83255461115769775635;
constexpr double HALF_LN_2PI = 0.91893853320467274178;
constexpr double kHighPwaic = 0.4;         // Vehtari, Gelman & Gabry (2017)

static_assert(kColPerThread * kColBlock == VAMP_PRED_MAX_SAMPLES && kColPerThread <= 32, "a thread's entries are a bit mask");

// LDS of one sample: line records and near-axis tables
__host__ __device__ constexpr int slot_doubles(int K) { return K * (kRec + vamp::DTAB_N); }
static_assert((size_t)kEvalWaves * slot_doubles(VAMP_PRED_MAX_COMPONENTS) * sizeof(double) <= 64 * 1024 &&
                  (size_t)kEvalWaves * (64 / vamp::kNarrowLanes) * slot_doubles(vamp::kNarrowMaxK) * sizeof(double) <= 64 * 1024,
              "a launch that asks for more than 64 KiB of LDS needs side::raise_lds_limit");

struct Item {                      // one (group, pixel range)
    const double* chain;           // the group's chain (device)
    const double* x;               // the range's abscissa, data and, with known noise, noise and its logarithm (device)
    const double* y;
    const double* noise;           // NULL: the sample's sd
    const double* ln_noise;
    double* ll;                    // the item's scratch
    uint8_t* bad;                  // the group's [S] flags
    long long ld;                  // stride of t, in doubles
    long long fs_s, fs_p;          // strides of the scratch
    int W, D, K, q;                // q = 3 (Gauss) or 4 (Voigt) parameters per line
    int S, np, lanes;              // lanes that own a sample (vamp::group_lanes)
};

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

__global__ __launch_bounds__(kEvalBlock) void k_pred_eval(const Item* __restrict__ items, const int2* __restrict__ tasks,
                                                          int region_doubles) {
    extern __shared__ double lds[];
    const int2 task = tasks[blockIdx.x];
    const Item I = items[task.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lanes = I.lanes;
    const vamp::LaneGroup lg = vamp::lane_group(lane, lanes);
    const int nsub = lg.nsub, sub = lg.sub, gl = lg.gl;
    const int K = I.K;
    double* rec = lds + (size_t)wave * region_doubles + (size_t)sub * slot_doubles(K);
    double* dtab = rec + K * kRec;
    const int s_end = min(task.y + kSamplesPerBlock, I.S);
    const bool voigt = I.q == 4, free_sd = I.noise == nullptr;
    const unsigned long long gmask = (lanes == 64 ? ~0ull : ((1ull << lanes) - 1ull)) << (sub * lanes);

    for (int sb = task.y + wave * nsub; sb < s_end; sb += kEvalWaves * nsub) {      // (uniform per wavefront)
        const int s = sb + sub;
        const bool valid = s < s_end;
        // 1. the sample's line records and its sd, once
        bool bad_lane = false;
        double sd = 1.0;
        if (valid) {
            const int t = s / I.W, w = s - t * I.W;
            const double* th = I.chain + (long long)t * I.ld + (long long)w * I.D;
            if (free_sd) {
                sd = th[I.D - 1];
                bad_lane = !isfinite(sd) || sd <= 0.0;
            }
            if (gl < K) {
                th += I.q * gl;
                const double a = th[0], c = th[1];
                double* r = rec + gl * kRec;
                r[0] = c;
                if (voigt) {
                    const double Lw = th[2], G = th[3];
                    bad_lane = bad_lane || !(isfinite(a) && isfinite(c) && isfinite(Lw) && isfinite(G)) || G <= 0.0 || Lw < 0.0;
                    const double rG = vamp::rcp_nr(G);
                    const double y = (Lw * SQRT_LN2) * rG;
                    r[1] = (2.0 * SQRT_LN2) * rG;
                    r[2] = y;
                    r[3] = a * y;                      // tau_k = A y sqrt(pi) H: the evaluator returns sqrt(pi) H
                    r[4] = vamp::core_pole_factor(y);
                    r[5] = vamp::core_hy(y);
                } else {
                    const double sg = th[2];
                    bad_lane = bad_lane || !(isfinite(a) && isfinite(c) && isfinite(sg)) || sg <= 0.0;
                    r[1] = 1.0 / sg; r[2] = 0.0; r[3] = a; r[4] = 0.0; r[5] = 0.0;
                }
            }
        }
        const bool bad = (__ballot(bad_lane) & gmask) != 0ull;
        const bool good = valid && !bad;
        if (valid && gl == 0) I.bad[s] = bad ? 1 : 0;
        lds_fence();
        if (good && voigt) vamp::fill_dtab<kRec>(dtab, rec, K, gl, lanes);
        lds_fence();
        // 2. the item's pixels
        if (good) {
            const double ln_sd = free_sd ? log(sd) : 0.0;
            double* out = I.ll + (long long)s * I.fs_s;
            for (int p = gl; p < I.np; p += lanes) {
                const double xi = I.x[p];
                double tau = 0.0;
                for (int k = 0; k < K; ++k) tau += vamp::line_tau(voigt, xi, rec + k * kRec, dtab + k * vamp::DTAB_N);
                const double sigma = free_sd ? sd : I.noise[p], ln_sigma = free_sd ? ln_sd : I.ln_noise[p];
                const double r = (I.y[p] - exp(-tau)) / sigma;
                out[(long long)p * I.fs_p] = -0.5 * (r * r) - ln_sigma - HALF_LN_2PI;
            }
        }
        lds_fence();                                   // the records are free for the next sample
    }
}

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
    size_t item0, item1;           // its items (and column sets)
    size_t etask0, etask1;         // its k_pred_eval workgroups
    size_t ctask0, ctask1;         // its k_pred_column workgroups
    int region_doubles = 0;        // LDS of a wavefront of k_pred_eval
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
    if (scratch_bytes < 0) return fail(fn + "scratch_bytes must not be negative");
    std::vector<int> Sg(n_groups), Dg(n_groups);
    long long tot_pix = 0, tot_noise = 0, tot_s = 0;
    int s_max = 0;
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (!base[g]) return fail(at + "NULL base pointer");
        if (!x[g]) return fail(at + "NULL abscissa");
        if (!flux[g]) return fail(at + "NULL flux");
        if (n_pix[g] <= 0) return fail(at + "n_pix must be positive");
        if (n_comp[g] < 1 || n_comp[g] > VAMP_PRED_MAX_COMPONENTS)
            return fail(at + "n_comp = " + std::to_string(n_comp[g]) + " is outside 1 .. " + std::to_string(VAMP_PRED_MAX_COMPONENTS));
        if (mode[g] == 2) return fail(at + "mode 2 (NBZ3) is not supported: pass the chain in the GAUSS3 (0) or VOIGT4 (1) layout");
        if (mode[g] != 0 && mode[g] != 1) return fail(at + "mode must be 0 (GAUSS3) or 1 (VOIGT4)");
        if (sample_sd[g] != 0 && sample_sd[g] != 1) return fail(at + "sample_sd must be 0 or 1");
        if (sample_sd[g] && noise[g]) return fail(at + "noise must be NULL when sample_sd is set: the chain's sd is the noise");
        if (!sample_sd[g] && !noise[g]) return fail(at + "NULL noise without sample_sd");
        if (n_keep[g] <= 0 || walkers[g] <= 0) return fail(at + "n_keep and walkers must be positive");
        const long long S = (long long)n_keep[g] * walkers[g];
        if (S > VAMP_PRED_MAX_SAMPLES)
            return fail(at + "n_keep * walkers = " + std::to_string(S) + " exceeds " + std::to_string(VAMP_PRED_MAX_SAMPLES) +
                        " (subsample in time: ld * step, ceil(n_keep / step))");
        Dg[g] = (mode[g] == 1 ? 4 : 3) * n_comp[g] + sample_sd[g];
        if (ld[g] < (int64_t)walkers[g] * Dg[g]) return fail(at + "ld < walkers * ndim");
        for (int p = 0; p < n_pix[g]; ++p) {
            if (!std::isfinite(x[g][p])) return fail(at + "the abscissa is not finite at pixel " + std::to_string(p));
            if (!std::isfinite(flux[g][p])) return fail(at + "the flux is not finite at pixel " + std::to_string(p));
            if (noise[g] && !(std::isfinite(noise[g][p]) && noise[g][p] > 0.0))
                return fail(at + "the noise is not finite and positive at pixel " + std::to_string(p));
        }
        Sg[g] = (int)S;
        s_max = Sg[g] > s_max ? Sg[g] : s_max;
        tot_pix += n_pix[g];
        tot_noise += noise[g] ? n_pix[g] : 0;
        tot_s += S;
    }
    if (tot_pix > (1LL << 30)) return fail(fn + "too many outputs");
    const long long cap = (scratch_bytes ? scratch_bytes : kDefaultScratch) / (long long)sizeof(double);
    if (cap < s_max)
        return fail(fn + "scratch_bytes = " + std::to_string(scratch_bytes) + " is less than one column of the largest group (" +
                    std::to_string((long long)s_max * (long long)sizeof(double)) + " bytes)");

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    // device view of every group's chain: staged (host input) or as given
    std::vector<const double*> dbase(base, base + n_groups);
    DevBuf staging;
    if (!is_device) {
        std::vector<long long> len(n_groups);
        for (int g = 0; g < n_groups; ++g) len[g] = chain_span(n_keep[g], ld[g], walkers[g], Dg[g]);
        if (stage_chains(len, base, st, staging, dbase)) return -1;
    }

    // one buffer of doubles: abscissae | data | noise | ln noise | per-pixel outputs | group outputs
    const long long o_x = 0, o_y = o_x + tot_pix, o_n = o_y + tot_pix, o_ln = o_n + tot_noise, o_lppd = o_ln + tot_noise,
                    o_lm = o_lppd + tot_pix, o_pw = o_lm + tot_pix, o_grp = o_pw + tot_pix, o_end = o_grp + 4ll * n_groups;
    std::vector<double> h_in((size_t)o_lppd);
    {
        long long op = 0, on = 0;
        for (int g = 0; g < n_groups; ++g) {
            for (int p = 0; p < n_pix[g]; ++p) {
                h_in[o_x + op + p] = x[g][p];
                h_in[o_y + op + p] = flux[g][p];
                if (noise[g]) {
                    h_in[o_n + on + p] = noise[g][p];
                    h_in[o_ln + on + p] = std::log(noise[g][p]);
                }
            }
            op += n_pix[g];
            on += noise[g] ? n_pix[g] : 0;
        }
    }
    DevBuf d_main, d_bad, d_counts, d_scratch;
    HIP_TRY(hipMalloc(&d_main.p, (size_t)o_end * sizeof(double)));
    HIP_TRY(hipMalloc(&d_bad.p, (size_t)tot_s));
    HIP_TRY(hipMalloc(&d_counts.p, (size_t)n_groups * 3 * sizeof(int32_t)));     // {n_used, n_bad} per group, then n_high
    HIP_TRY(hipMemcpyAsync(d_main.p, h_in.data(), h_in.size() * sizeof(double), hipMemcpyHostToDevice, st));
    double* dm = d_main.as<double>();

    // the plan: items packed greedily into passes; a group that does not fit what is left of a pass is split over
    // pixel ranges
    std::vector<Item> items;
    std::vector<ColSet> sets;
    std::vector<Totals> totals;
    std::vector<int2> etasks, ctasks;
    std::vector<Pass> passes;
    std::vector<long long> item_scratch;                 // offset into the pass's scratch
    long long scratch_len = 0;
    {
        Pass cur{};
        long long used = 0, pix_off = 0, noise_off = 0, s_off = 0;
        auto close = [&]() {
            cur.item1 = items.size(); cur.etask1 = etasks.size(); cur.ctask1 = ctasks.size();
            if (cur.item1 > cur.item0) passes.push_back(cur);
            scratch_len = used > scratch_len ? used : scratch_len;
            cur = Pass{};
            cur.item0 = items.size(); cur.etask0 = etasks.size(); cur.ctask0 = ctasks.size();
            used = 0;
        };
        for (int g = 0; g < n_groups; ++g) {
            const int S = Sg[g], K = n_comp[g], P = n_pix[g];
            const int lanes = vamp::group_lanes(VAMP_PRED_NARROW, P, K);
            const int region = (64 / lanes) * slot_doubles(K);
            uint8_t* bad = d_bad.as<uint8_t>() + s_off;
            for (int p0 = 0; p0 < P;) {
                const long long fit = (cap - used) / S;
                if (fit == 0) { close(); continue; }              // (an empty pass holds at least one column: cap >= s_max)
                const int np = (int)((long long)(P - p0) < fit ? (P - p0) : fit);
                Item it;
                it.chain = dbase[g];
                it.x = dm + o_x + pix_off + p0;
                it.y = dm + o_y + pix_off + p0;
                it.noise = noise[g] ? dm + o_n + noise_off + p0 : nullptr;
                it.ln_noise = noise[g] ? dm + o_ln + noise_off + p0 : nullptr;
                it.ll = nullptr;                                   // (the scratch is allocated when its size is known)
                it.bad = bad;
                it.ld = ld[g];
                it.fs_s = VAMP_PRED_PIXEL_MAJOR ? 1 : np;
                it.fs_p = VAMP_PRED_PIXEL_MAJOR ? S : 1;
                it.W = walkers[g]; it.D = Dg[g]; it.K = K; it.q = mode[g] == 1 ? 4 : 3;
                it.S = S; it.np = np; it.lanes = lanes;
                ColSet cs;
                cs.src = nullptr; cs.bad = bad;
                cs.lppd = dm + o_lppd + pix_off + p0;
                cs.ll_mean = dm + o_lm + pix_off + p0;
                cs.pwaic = dm + o_pw + pix_off + p0;
                cs.counts = p0 == 0 ? d_counts.as<int32_t>() + 2 * g : nullptr;
                cs.stride_c = it.fs_p; cs.stride_s = it.fs_s; cs.S = S;
                item_scratch.push_back(used);
                const int ii = (int)items.size();
                items.push_back(it);
                sets.push_back(cs);
                for (int s0 = 0; s0 < S; s0 += kSamplesPerBlock) etasks.push_back(make_int2(ii, s0));
                for (int c = 0; c < np; ++c) ctasks.push_back(make_int2(ii, c));
                cur.region_doubles = region > cur.region_doubles ? region : cur.region_doubles;
                used += (long long)np * S;
                p0 += np;
            }
            Totals t;
            t.lppd = dm + o_lppd + pix_off; t.ll_mean = dm + o_lm + pix_off; t.pwaic = dm + o_pw + pix_off; t.P = P;
            totals.push_back(t);
            pix_off += P; noise_off += noise[g] ? P : 0; s_off += S;
        }
        close();
    }
    if (etasks.size() > 0x7fffffff || ctasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");
    HIP_TRY(hipMalloc(&d_scratch.p, (size_t)scratch_len * sizeof(double)));
    for (size_t i = 0; i < items.size(); ++i) {
        items[i].ll = d_scratch.as<double>() + item_scratch[i];
        sets[i].src = items[i].ll;
    }

    DevBuf d_items, d_sets, d_totals, d_etasks, d_ctasks;
    if (upload(d_items, items, st) || upload(d_sets, sets, st) || upload(d_totals, totals, st) || upload(d_etasks, etasks, st) ||
        upload(d_ctasks, ctasks, st))
        return -1;
    for (const Pass& ps : passes) {
        hipLaunchKernelGGL(k_pred_eval, dim3((unsigned)(ps.etask1 - ps.etask0)), dim3(kEvalBlock),
                           (size_t)kEvalWaves * ps.region_doubles * sizeof(double), st, d_items.as<Item>(),
                           d_etasks.as<int2>() + ps.etask0, ps.region_doubles);
        HIP_TRY(hipGetLastError());
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
    std::vector<int32_t> counts((size_t)n_groups * 2);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < n_groups; ++g) {
        if (n_used) n_used[g] = counts[2 * g];
        if (n_bad) n_bad[g] = counts[2 * g + 1];
    }
    return 0;
}
