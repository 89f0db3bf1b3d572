// posterior.hip -- posterior flux band and equivalent-width summaries of ensemble chains
// (include/vamp_post.h, libvamp_post.so).  Definitions: DESIGN.md "Posterior summaries".
//
// The work is a list of items (group, pixel range), packed greedily into passes whose flux scratch fits
// scratch_bytes (chain_groups.hpp, which predictive.hip shares).  Two launches per pass:
//   k_post_eval    one workgroup per (item, 64 samples).  A wavefront -- or, for short regions of few lines, a
//                  16-lane group -- owns a sample: its parameters become line records once (centre, scale,
//                  damping, amplitude factor, pole factor, h y and the 44-entry near-axis table of voigt_math.hpp, in
//                  LDS), then its lanes walk the item's pixels with the evaluator of k_model, write the flux to the
//                  scratch matrix and hand their decrements 1 - exp(-tau_k), 1 - flux to the lanes 0 .. K, which add
//                  them IN PIXEL ORDER to the sample's row of the group's [S, K + 1] equivalent-width buffer (plain
//                  read-add-write: a region split over passes continues the same sum, so it does not depend on the
//                  packing).
//   k_post_column  one workgroup per column (a pixel's flux over the samples; once per group, its K + 1
//                  equivalent-width columns): the column in LDS, bad samples and the padding to the next power of
//                  two +inf, a bitonic sort, then the mean, the centred standard deviation and the quantiles of
//                  the first n entries.
// Everything is fp64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_post.h"
#include "chain_groups.hpp"
#include "lane_group.hpp"
#include "side_call.hpp"
#include "voigt_math.hpp"

#define VAMP_POST_API extern "C" __attribute__((visibility("default")))

// Orientation of the flux scratch of an item ([S samples] x [np pixels]):
//   0  sample-major, flux[s * np + p]: the evaluation's stores are contiguous, the column loads strided
//   1  pixel-major,  flux[p * S + s]: the column loads are contiguous, the evaluation's stores strided
// and whether a 16-lane group may own a sample.  Both decided by measurement (profiles/posterior_bench.txt, q1422 shape,
// ms per call): sample-major 35.13 against pixel-major 35.43 -- no difference, neither kernel is bound by HBM, the
// contiguous stores stay; 16-lane groups 35.13 against 36.88 without -- used.
#ifndef VAMP_POST_PIXEL_MAJOR
#define VAMP_POST_PIXEL_MAJOR 0
#endif
#ifndef VAMP_POST_NARROW
#define VAMP_POST_NARROW 1
#endif

namespace {

using namespace vamp::side;
using vamp::lds_fence;

constexpr int kEvalBlock = 256;            // four wavefronts
constexpr int kEvalWaves = kEvalBlock / 64;
constexpr int kSamplesPerBlock = 64;
constexpr int kRec = 6;                    // doubles of a line record
constexpr int kColBlock = 1024;            // one size for every column: the reduction order must not depend on the pass

// LDS of one sample: line records, near-axis tables, and the [K + 1][lanes + 1] tile the decrements cross lanes in
// (rows padded by one: the summing lanes read down a column each)
__host__ __device__ constexpr int slot_doubles(int K, int lanes) { return K * (kRec + vamp::DTAB_N) + (K + 1) * (lanes + 1); }

struct Item {                      // one (group, pixel range)
    const double* chain;           // the group's chain (device)
    const double* x;               // the range's abscissa (device)
    double* flux;                  // the item's scratch
    double* ew;                    // the group's [S][K + 1] decrement sums
    uint8_t* bad;                  // the group's [S] flags
    long long ld;                  // stride of t, in doubles
    long long fs_s, fs_p;          // strides of the scratch
    int W, D, K, q;                // q = 3 (Gauss) or 4 (Voigt) parameters per line
    int S, np, p0, lanes;          // lanes that own a sample (vamp::group_lanes)
};

struct ColSet {                    // columns that share a source matrix
    const double* src;             // value of (column c, sample s) = src[c * stride_c + s * stride_s] * scale
    const uint8_t* bad;
    double* mean;                  // [c]
    double* sd;                    // [c]
    double* q;                     // [qi * q_qs + c * q_cs]
    int32_t* counts;               // {n_used, n_bad} of the group, or NULL
    long long stride_c, stride_s, q_qs, q_cs;
    double scale;
    int S, n2;                     // n2: S rounded up to a power of two
};

__global__ __launch_bounds__(kEvalBlock) void k_post_eval(const Item* __restrict__ items, const int2* __restrict__ tasks,
                                                          int region_doubles) {
    extern __shared__ double lds[];
    const int2 task = tasks[blockIdx.x];
    const Item I = items[task.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lanes = I.lanes;
    const vamp::LaneGroup lg = vamp::lane_group(lane, lanes);
    const int nsub = lg.nsub, sub = lg.sub, gl = lg.gl;
    const int K = I.K, row = lanes + 1;
    double* rec = lds + (size_t)wave * region_doubles + (size_t)sub * slot_doubles(K, lanes);
    double* dtab = rec + K * kRec;
    double* tile = dtab + K * vamp::DTAB_N;
    const int s_end = min(task.y + kSamplesPerBlock, I.S);
    const bool voigt = I.q == 4;
    const unsigned long long gmask = vamp::group_mask(lanes, sub);

    for (int sb = task.y + wave * nsub; sb < s_end; sb += kEvalWaves * nsub) {      // (uniform per wavefront)
        const int s = sb + sub;
        const bool valid = s < s_end;
        // 1. the sample's line records, once
        bool bad_lane = false;
        if (valid && gl < K) {
            const int t = s / I.W, w = s - t * I.W;
            bad_lane = vamp::line_record(voigt, I.chain + (long long)t * I.ld + (long long)w * I.D + I.q * gl, rec + gl * kRec);
        }
        const bool bad = (__ballot(bad_lane) & gmask) != 0ull;
        const bool good = valid && !bad;
        if (valid && gl == 0) I.bad[s] = bad ? 1 : 0;
        lds_fence();
        if (good && voigt) vamp::fill_dtab<kRec>(dtab, rec, K, gl, lanes);
        lds_fence();
        // 2. the item's pixels, a round of `lanes` at a time; lanes 0 .. K keep the running sums
        const bool owner = good && gl <= K;
        double* ew = I.ew + (long long)s * (K + 1) + gl;
        double acc = (owner && I.p0 > 0) ? *ew : 0.0;
        for (int r0 = 0; r0 < I.np; r0 += lanes) {
            const int p = r0 + gl;
            if (good && p < I.np) {
                const double xi = I.x[p];
                double tau = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double tk = vamp::line_tau(voigt, xi, rec + k * kRec, dtab + k * vamp::DTAB_N);
                    tile[k * row + gl] = 1.0 - exp(-tk);
                    tau += tk;
                }
                const double f = exp(-tau);
                I.flux[(long long)s * I.fs_s + (long long)p * I.fs_p] = f;
                tile[K * row + gl] = 1.0 - f;
            }
            lds_fence();
            if (owner) {
                const int n = min(lanes, I.np - r0);
                for (int j = 0; j < n; ++j) acc += tile[gl * row + j];
            }
            lds_fence();
        }
        if (owner) *ew = acc;
    }
}

// Dynamic LDS: n2 doubles.
__global__ __launch_bounds__(kColBlock) void k_post_column(const ColSet* __restrict__ sets, const int2* __restrict__ tasks,
                                                           const double* __restrict__ probs, int Q) {
    extern __shared__ double col[];
    __shared__ double red[kColBlock];
    const int2 task = tasks[blockIdx.x];
    const ColSet C = sets[task.x];
    const int c = task.y, tid = threadIdx.x, n2 = C.n2;
    const double* src = C.src + (long long)c * C.stride_c;

    double nb = 0.0, nn = 0.0;
    for (int i = tid; i < n2; i += kColBlock) {
        double v = INFINITY;
        if (i < C.S) {
            if (C.bad[i]) nb += 1.0;
            else {
                v = src[(long long)i * C.stride_s] * C.scale;
                if (isnan(v)) { nn += 1.0; v = INFINITY; }
            }
        }
        col[i] = v;
    }
    const int n_bad = (int)vamp::block_sum<kColBlock>(nb, red);       // (ends with a barrier: the column is staged)
    const int n_nan = (int)vamp::block_sum<kColBlock>(nn, red);
    const int n = C.S - n_bad;

    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += kColBlock) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const double a = col[i], b = col[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { col[i] = b; col[l] = a; }
            }
            __syncthreads();
        }

    double part = 0.0;
    for (int i = tid; i < n; i += kColBlock) part += col[i];
    const double mean = vamp::block_sum<kColBlock>(part, red) / (double)n;
    part = 0.0;
    for (int i = tid; i < n; i += kColBlock) { const double d = col[i] - mean; part = fma(d, d, part); }
    const double var = vamp::block_sum<kColBlock>(part, red) / (double)n;
    const bool none = n == 0 || n_nan > 0;           // a NaN among the values makes every statistic NaN, as in numpy

    if (tid == 0) {
        C.mean[c] = none ? NAN : mean;
        C.sd[c] = none ? NAN : sqrt(var);
        if (C.counts) { C.counts[0] = n; C.counts[1] = n_bad; }
    }
    if (tid < Q) {
        double v = NAN;
        if (!none) {
            // numpy's arithmetic, one rounding per operation.  Fused, t = fma(n - 1, p, -lo) keeps the unrounded product:
            // at n = 21, p = 0.975 that is 0.5 - 4e-16 where numpy has 0.5, which picks the other form of the interpolation
            // below -- +inf where numpy has NaN when the upper order statistic is infinite
#pragma clang fp contract(off)
            const double h = (double)(n - 1) * probs[tid];
            int lo = (int)floor(h);
            lo = lo < n - 1 ? lo : n - 1;
            const int hi = lo + 1 < n ? lo + 1 : n - 1;
            const double a = col[lo], b = col[hi], t = h - (double)lo, d = b - a;
            // numpy's _lerp, with no shortcut for lo == hi (p = 1, n = 1): an infinite order statistic that is hit
            // exactly gives inf - inf = NaN there, and so it does here
            v = t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
        }
        C.q[(long long)tid * C.q_qs + (long long)c * C.q_cs] = v;
    }
}

constexpr size_t kColMaxLds = (size_t)VAMP_POST_MAX_SAMPLES * sizeof(double);
constexpr size_t kEvalMaxLds = (size_t)kEvalWaves * slot_doubles(VAMP_POST_MAX_COMPONENTS, 64) * sizeof(double);
struct Pass {
    size_t etask0, etask1;        // its k_post_eval workgroups
    size_t ctask0, ctask1;         // its k_post_column workgroups
    int region_doubles = 0;        // LDS of a wavefront of k_post_eval
    int n2 = 1;                    // longest column
};

}  // namespace

VAMP_POST_API int vamp_post_version(void) { return VAMP_POST_ABI_VERSION; }

VAMP_POST_API const char* vamp_post_last_error(void) { return g_err.c_str(); }

VAMP_POST_API int vamp_post_summaries(int device, void* hip_stream, int n_groups, const double* const* x, const int32_t* n_pix,
                                      const int32_t* n_comp, const int32_t* mode, const int32_t* sample_sd,
                                      const double* const* base, int is_device, const int64_t* ld, const int32_t* n_keep,
                                      const int32_t* walkers, const double* pixel_width, int n_probs, const double* probs,
                                      int64_t scratch_bytes, double* flux_mean, double* flux_sd, double* flux_q, double* ew_mean,
                                      double* ew_sd, double* ew_q, double* comp_ew_mean, double* comp_ew_sd, double* comp_ew_q,
                                      int32_t* n_used, int32_t* n_bad) {
    g_err.clear();
    const std::string fn = "vamp_post_summaries: ";
    if (n_groups <= 0) return fail(fn + "n_groups must be positive");
    if (!x || !n_pix || !n_comp || !mode || !sample_sd || !base || !ld || !n_keep || !walkers || !pixel_width || !probs)
        return fail(fn + "NULL argument");
    if (n_probs < 1 || n_probs > VAMP_POST_MAX_PROBS)
        return fail(fn + "n_probs = " + std::to_string(n_probs) + " is outside 1 .. " + std::to_string(VAMP_POST_MAX_PROBS));
    for (int i = 0; i < n_probs; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return fail(fn + "probs[" + std::to_string(i) + "] is outside [0, 1]");
    const int Q = n_probs;
    ChainGroups cg;
    const std::string err = check_chain_groups(fn, n_groups, x, n_pix, n_comp, mode, sample_sd, base, ld, n_keep, walkers, scratch_bytes,
                                               VAMP_POST_MAX_SAMPLES, VAMP_POST_MAX_COMPONENTS,
                                               "a column must fit the LDS; subsample in time: ld * step, ceil(n_keep / step)", cg);
    if (!err.empty()) return fail(err);
    const long long tot_pix = cg.tot_pix, tot_s = cg.tot_s;
    long long tot_comp = 0, tot_ew = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (!std::isfinite(pixel_width[g])) return fail(fn + "group " + std::to_string(g) + ": pixel_width is not finite");
        tot_comp += n_comp[g];
        tot_ew += (long long)cg.S[g] * (n_comp[g] + 1);
    }
    if (tot_pix * Q > (1LL << 31) || tot_pix > (1LL << 30)) return fail(fn + "too many outputs");

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    // both kernels may ask for more dynamic LDS than a launch gets by default
    if (raise_lds_limit(fn, device, {{reinterpret_cast<const void*>(&k_post_column), kColMaxLds},
                                     {reinterpret_cast<const void*>(&k_post_eval), kEvalMaxLds}}))
        return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    // device view of every group's chain: staged (host input) or as given
    std::vector<const double*> dbase(base, base + n_groups);
    DevBuf staging;
    if (!is_device) {
        std::vector<long long> len(n_groups);
        for (int g = 0; g < n_groups; ++g) len[g] = chain_span(n_keep[g], ld[g], walkers[g], cg.D[g]);
        if (stage_chains(len, base, st, staging, dbase)) return -1;
    }

    // one buffer of doubles: abscissae | decrement sums | outputs; one of bytes (bad flags); one of counts
    const long long o_x = 0, o_ew = o_x + tot_pix, o_out = o_ew + tot_ew;
    const long long o_fm = o_out, o_fs = o_fm + tot_pix, o_fq = o_fs + tot_pix, o_em = o_fq + tot_pix * Q, o_es = o_em + n_groups,
                    o_eq = o_es + n_groups, o_cm = o_eq + (long long)n_groups * Q, o_cs = o_cm + tot_comp, o_cq = o_cs + tot_comp,
                    o_end = o_cq + tot_comp * Q;
    DevBuf d_main, d_bad, d_counts, d_probs, d_scratch;
    HIP_TRY(hipMalloc(&d_main.p, (size_t)o_end * sizeof(double)));
    HIP_TRY(hipMalloc(&d_bad.p, (size_t)tot_s));
    HIP_TRY(hipMalloc(&d_counts.p, (size_t)n_groups * 2 * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&d_probs.p, (size_t)Q * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(d_probs.p, probs, (size_t)Q * sizeof(double), hipMemcpyHostToDevice, st));
    double* dm = d_main.as<double>();
    {
        long long o = 0;
        for (int g = 0; g < n_groups; ++g) {
            HIP_TRY(hipMemcpyAsync(dm + o_x + o, x[g], (size_t)n_pix[g] * sizeof(double), hipMemcpyHostToDevice, st));
            o += n_pix[g];
        }
    }

    // the plan (chain_groups.hpp): one item and one column set per range; the K + 1 equivalent-width columns of a
    // group follow its last range, in that range's pass: they run after the k_post_eval that completes their sums
    const PassPlan plan = plan_passes(cg.cap, cg.S, n_pix, n_groups);
    const long long scratch_len = plan.scratch_len;
    HIP_TRY(hipMalloc(&d_scratch.p, (size_t)scratch_len * sizeof(double)));
    std::vector<Item> items;
    std::vector<ColSet> sets;
    std::vector<int2> etasks, ctasks;
    std::vector<Pass> passes(plan.first.size());
    long long pix_off = 0, ew_off = 0, s_off = 0, comp_off = 0;      // of the range's group
    for (const Range& r : plan.ranges) {
        const int g = r.group, S = cg.S[g], K = n_comp[g], P = n_pix[g], p0 = r.p0, np = r.np;
        int n2 = 1;
        while (n2 < S) n2 <<= 1;
        const int lanes = vamp::group_lanes(VAMP_POST_NARROW, P, K);
        const int region = (64 / lanes) * slot_doubles(K, lanes);
        Pass& ps = passes[r.pass];
        if (r.offset == 0) { ps.etask0 = etasks.size(); ps.ctask0 = ctasks.size(); }
        Item it;
        it.chain = dbase[g];
        it.x = dm + o_x + pix_off + p0;
        it.flux = d_scratch.as<double>() + r.offset;
        it.ew = dm + o_ew + ew_off; it.bad = d_bad.as<uint8_t>() + s_off;
        it.ld = ld[g];
        it.fs_s = VAMP_POST_PIXEL_MAJOR ? 1 : np;
        it.fs_p = VAMP_POST_PIXEL_MAJOR ? S : 1;
        it.W = walkers[g]; it.D = cg.D[g]; it.K = K; it.q = mode[g] == 1 ? 4 : 3;
        it.S = S; it.np = np; it.p0 = p0; it.lanes = lanes;
        ColSet cs;
        cs.src = it.flux; cs.bad = it.bad;
        cs.mean = dm + o_fm + pix_off + p0;
        cs.sd = dm + o_fs + pix_off + p0;
        cs.q = dm + o_fq + pix_off * Q + p0;
        cs.counts = nullptr;
        cs.stride_c = it.fs_p; cs.stride_s = it.fs_s; cs.q_qs = P; cs.q_cs = 1;
        cs.scale = 1.0; cs.S = S; cs.n2 = n2;
        const int ii = (int)items.size(), si = (int)sets.size();
        items.push_back(it);
        sets.push_back(cs);
        for (int s0 = 0; s0 < S; s0 += kSamplesPerBlock) etasks.push_back(make_int2(ii, s0));
        for (int c = 0; c < np; ++c) ctasks.push_back(make_int2(si, c));
        ps.region_doubles = region > ps.region_doubles ? region : ps.region_doubles;
        ps.n2 = n2 > ps.n2 ? n2 : ps.n2;
        if (p0 + np == P) {
            ColSet comp;                                           // the lines' columns, then the region's
            comp.src = it.ew; comp.bad = it.bad;
            comp.mean = dm + o_cm + comp_off; comp.sd = dm + o_cs + comp_off; comp.q = dm + o_cq + comp_off * Q;
            comp.counts = nullptr;
            comp.stride_c = 1; comp.stride_s = K + 1; comp.q_qs = 1; comp.q_cs = Q;
            comp.scale = pixel_width[g]; comp.S = S; comp.n2 = n2;
            ColSet tot = comp;
            tot.src = it.ew + K;
            tot.mean = dm + o_em + g; tot.sd = dm + o_es + g; tot.q = dm + o_eq + (long long)g * Q;
            tot.counts = d_counts.as<int32_t>() + 2 * g;
            sets.push_back(comp);
            sets.push_back(tot);
            for (int k = 0; k < K; ++k) ctasks.push_back(make_int2(si + 1, k));
            ctasks.push_back(make_int2(si + 2, 0));
            pix_off += P; ew_off += (long long)S * (K + 1); s_off += S; comp_off += K;
        }
        ps.etask1 = etasks.size(); ps.ctask1 = ctasks.size();
    }
    if (etasks.size() > 0x7fffffff || ctasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");

    DevBuf d_items, d_sets, d_etasks, d_ctasks;
    if (upload(d_items, items, st) || upload(d_sets, sets, st) || upload(d_etasks, etasks, st) || upload(d_ctasks, ctasks, st)) return -1;
    for (const Pass& ps : passes) {
        hipLaunchKernelGGL(k_post_eval, dim3((unsigned)(ps.etask1 - ps.etask0)), dim3(kEvalBlock),
                           (size_t)kEvalWaves * ps.region_doubles * sizeof(double), st, d_items.as<Item>(),
                           d_etasks.as<int2>() + ps.etask0, ps.region_doubles);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_post_column, dim3((unsigned)(ps.ctask1 - ps.ctask0)), dim3(kColBlock), (size_t)ps.n2 * sizeof(double), st,
                           d_sets.as<ColSet>(), d_ctasks.as<int2>() + ps.ctask0, d_probs.as<double>(), Q);
        HIP_TRY(hipGetLastError());
    }

    const long long sz = sizeof(double);
    if (fetch(flux_mean, dm + o_fm, tot_pix * sz, st) || fetch(flux_sd, dm + o_fs, tot_pix * sz, st) ||
        fetch(flux_q, dm + o_fq, tot_pix * Q * sz, st) || fetch(ew_mean, dm + o_em, n_groups * sz, st) ||
        fetch(ew_sd, dm + o_es, n_groups * sz, st) || fetch(ew_q, dm + o_eq, (long long)n_groups * Q * sz, st) ||
        fetch(comp_ew_mean, dm + o_cm, tot_comp * sz, st) || fetch(comp_ew_sd, dm + o_cs, tot_comp * sz, st) ||
        fetch(comp_ew_q, dm + o_cq, tot_comp * Q * sz, st))
        return -1;
    return fetch_counts(d_counts, n_groups, n_used, n_bad, st);
}
