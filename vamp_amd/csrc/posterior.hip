// posterior.hip -- posterior flux band and equivalent-width summaries of ensemble chains
// (include/vamp_post.h, libvamp_post.so).  Definitions: DESIGN.md "Posterior summaries".
//
// The work is a list of items (group, pixel range), packed greedily into passes whose flux scratch fits
// scratch_bytes.  Two launches per pass:
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
constexpr long long kDefaultScratch = 256ll << 20;
constexpr double SQRT_LN2 = 0.83255461115769775635;

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

// The group geometry, the table fill and the optical depth of a line are written out here, not taken from
// lane_group.hpp: through the header's functions the compiler orders this kernel's loads differently and renumbers
// its registers (code 8472 -> 8488 bytes; 128 VGPRs, 100 SGPRs, occupancy 4, no scratch either way), and that form has
// not been timed or compared bit for bit on a device.  eval_point of evidence.hip compiles to the same code both ways.
__global__ __launch_bounds__(kEvalBlock) void k_post_eval(const Item* __restrict__ items, const int2* __restrict__ tasks,
                                                          int region_doubles) {
    extern __shared__ double lds[];
    const int2 task = tasks[blockIdx.x];
    const Item I = items[task.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lanes = I.lanes, nsub = 64 / lanes;
    const int sub = lane / lanes, gl = lane - sub * lanes;
    const int K = I.K, row = lanes + 1;
    double* rec = lds + (size_t)wave * region_doubles + (size_t)sub * slot_doubles(K, lanes);
    double* dtab = rec + K * kRec;
    double* tile = dtab + K * vamp::DTAB_N;
    const int s_end = min(task.y + kSamplesPerBlock, I.S);
    const bool voigt = I.q == 4;
    const unsigned long long gmask = (lanes == 64 ? ~0ull : ((1ull << lanes) - 1ull)) << (sub * lanes);

    for (int sb = task.y + wave * nsub; sb < s_end; sb += kEvalWaves * nsub) {      // (uniform per wavefront)
        const int s = sb + sub;
        const bool valid = s < s_end;
        // 1. the sample's line records, once
        bool bad_lane = false;
        if (valid && gl < K) {
            const int t = s / I.W, w = s - t * I.W;
            const double* th = I.chain + (long long)t * I.ld + (long long)w * I.D + I.q * gl;
            const double a = th[0], c = th[1];
            double* r = rec + gl * kRec;
            r[0] = c;
            if (voigt) {
                const double Lw = th[2], G = th[3];
                bad_lane = !(isfinite(a) && isfinite(c) && isfinite(Lw) && isfinite(G)) || G <= 0.0 || Lw < 0.0;
                const double rG = vamp::rcp_nr(G);
                const double y = (Lw * SQRT_LN2) * rG;
                r[1] = (2.0 * SQRT_LN2) * rG;
                r[2] = y;
                r[3] = a * y;                      // tau_k = A y sqrt(pi) H: the evaluator returns sqrt(pi) H
                r[4] = vamp::core_pole_factor(y);
                r[5] = vamp::core_hy(y);
            } else {
                const double sg = th[2];
                bad_lane = !(isfinite(a) && isfinite(c) && isfinite(sg)) || sg <= 0.0;
                r[1] = 1.0 / sg; r[2] = 0.0; r[3] = a; r[4] = 0.0; r[5] = 0.0;
            }
        }
        const bool bad = (__ballot(bad_lane) & gmask) != 0ull;
        const bool good = valid && !bad;
        if (valid && gl == 0) I.bad[s] = bad ? 1 : 0;
        lds_fence();
        if (good && voigt)
            for (int e = gl; e < K * vamp::DTAB_N; e += lanes) {
                const int k = e / vamp::DTAB_N, n = e - k * vamp::DTAB_N;
                dtab[e] = vamp::core_dtab_entry(n, rec[k * kRec + 2]);
            }
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
                    const double* r = rec + k * kRec;
                    double tk;
                    if (voigt) {
                        const double X = fabs(xi - r[0]) * r[1];
                        tk = r[3] * vamp::voigt_Hs(X, r[2], dtab + k * vamp::DTAB_N, r[4], r[5]);
                    } else {
                        const double u = (xi - r[0]) * r[1];
                        tk = r[3] * exp(-0.5 * (u * u));
                    }
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
    size_t item0, item1;           // its items
    size_t etask0, etask1;         // its k_post_eval workgroups
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
    if (scratch_bytes < 0) return fail(fn + "scratch_bytes must not be negative");
    const int Q = n_probs;
    std::vector<int> Sg(n_groups), Dg(n_groups);
    long long tot_pix = 0, tot_comp = 0, tot_ew = 0, tot_s = 0;
    int s_max = 0;
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (!base[g]) return fail(at + "NULL base pointer");
        if (!x[g]) return fail(at + "NULL abscissa");
        if (n_pix[g] <= 0) return fail(at + "n_pix must be positive");
        if (n_comp[g] < 1 || n_comp[g] > VAMP_POST_MAX_COMPONENTS)
            return fail(at + "n_comp = " + std::to_string(n_comp[g]) + " is outside 1 .. " + std::to_string(VAMP_POST_MAX_COMPONENTS));
        if (mode[g] == 2) return fail(at + "mode 2 (NBZ3) is not supported: pass the chain in the GAUSS3 (0) or VOIGT4 (1) layout");
        if (mode[g] != 0 && mode[g] != 1) return fail(at + "mode must be 0 (GAUSS3) or 1 (VOIGT4)");
        if (sample_sd[g] != 0 && sample_sd[g] != 1) return fail(at + "sample_sd must be 0 or 1");
        if (n_keep[g] <= 0 || walkers[g] <= 0) return fail(at + "n_keep and walkers must be positive");
        const long long S = (long long)n_keep[g] * walkers[g];
        if (S > VAMP_POST_MAX_SAMPLES)
            return fail(at + "n_keep * walkers = " + std::to_string(S) + " exceeds " + std::to_string(VAMP_POST_MAX_SAMPLES) +
                        " (a column must fit the LDS; subsample in time: ld * step, ceil(n_keep / step))");
        Dg[g] = (mode[g] == 1 ? 4 : 3) * n_comp[g] + sample_sd[g];
        if (ld[g] < (int64_t)walkers[g] * Dg[g]) return fail(at + "ld < walkers * ndim");
        if (!std::isfinite(pixel_width[g])) return fail(at + "pixel_width is not finite");
        for (int p = 0; p < n_pix[g]; ++p)
            if (!std::isfinite(x[g][p])) return fail(at + "the abscissa is not finite at pixel " + std::to_string(p));
        Sg[g] = (int)S;
        s_max = Sg[g] > s_max ? Sg[g] : s_max;
        tot_pix += n_pix[g];
        tot_comp += n_comp[g];
        tot_ew += S * (n_comp[g] + 1);
        tot_s += S;
    }
    if (tot_pix * Q > (1LL << 31) || tot_pix > (1LL << 30)) return fail(fn + "too many outputs");
    const long long cap = (scratch_bytes ? scratch_bytes : kDefaultScratch) / (long long)sizeof(double);
    if (cap < s_max)
        return fail(fn + "scratch_bytes = " + std::to_string(scratch_bytes) + " is less than one column of the largest group (" +
                    std::to_string((long long)s_max * (long long)sizeof(double)) + " bytes)");

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
        for (int g = 0; g < n_groups; ++g) len[g] = chain_span(n_keep[g], ld[g], walkers[g], Dg[g]);
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

    // the plan: items packed greedily into passes; a group that does not fit what is left of a pass is split over
    // pixel ranges; the K + 1 equivalent-width columns of a group follow its last range
    std::vector<Item> items;
    std::vector<ColSet> sets;
    std::vector<int2> etasks, ctasks;
    std::vector<Pass> passes;
    std::vector<long long> item_scratch, set_scratch;    // offset into the pass's scratch (a set off the scratch: -1)
    long long scratch_len = 0;
    {
        Pass cur{};
        long long used = 0, pix_off = 0, ew_off = 0, s_off = 0, comp_off = 0;
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
            int n2 = 1;
            while (n2 < S) n2 <<= 1;
            const int lanes = vamp::group_lanes(VAMP_POST_NARROW, P, K);
            const int region = (64 / lanes) * slot_doubles(K, lanes);
            double* ew = dm + o_ew + ew_off;
            uint8_t* bad = d_bad.as<uint8_t>() + s_off;
            for (int p0 = 0; p0 < P;) {
                const long long fit = (cap - used) / S;
                if (fit == 0) { close(); continue; }              // (an empty pass holds at least one column: cap >= s_max)
                const int np = (int)((long long)(P - p0) < fit ? (P - p0) : fit);
                Item it;
                it.chain = dbase[g];
                it.x = dm + o_x + pix_off + p0;
                it.flux = nullptr;                                 // (the scratch is allocated when its size is known)
                it.ew = ew; it.bad = bad;
                it.ld = ld[g];
                it.fs_s = VAMP_POST_PIXEL_MAJOR ? 1 : np;
                it.fs_p = VAMP_POST_PIXEL_MAJOR ? S : 1;
                it.W = walkers[g]; it.D = Dg[g]; it.K = K; it.q = mode[g] == 1 ? 4 : 3;
                it.S = S; it.np = np; it.p0 = p0; it.lanes = lanes;
                ColSet cs;
                cs.src = nullptr; cs.bad = bad;
                cs.mean = dm + o_fm + pix_off + p0;
                cs.sd = dm + o_fs + pix_off + p0;
                cs.q = dm + o_fq + pix_off * Q + p0;
                cs.counts = nullptr;
                cs.stride_c = it.fs_p; cs.stride_s = it.fs_s; cs.q_qs = P; cs.q_cs = 1;
                cs.scale = 1.0; cs.S = S; cs.n2 = n2;
                item_scratch.push_back(used);
                set_scratch.push_back(used);
                const int ii = (int)items.size(), si = (int)sets.size();
                items.push_back(it);
                sets.push_back(cs);
                for (int s0 = 0; s0 < S; s0 += kSamplesPerBlock) etasks.push_back(make_int2(ii, s0));
                for (int c = 0; c < np; ++c) ctasks.push_back(make_int2(si, c));
                cur.region_doubles = region > cur.region_doubles ? region : cur.region_doubles;
                cur.n2 = n2 > cur.n2 ? n2 : cur.n2;
                used += (long long)np * S;
                p0 += np;
            }
            ColSet comp;                                           // the lines' columns, then the region's
            comp.src = ew; comp.bad = bad;
            comp.mean = dm + o_cm + comp_off; comp.sd = dm + o_cs + comp_off; comp.q = dm + o_cq + comp_off * Q;
            comp.counts = nullptr;
            comp.stride_c = 1; comp.stride_s = K + 1; comp.q_qs = 1; comp.q_cs = Q;
            comp.scale = pixel_width[g]; comp.S = S; comp.n2 = n2;
            ColSet tot = comp;
            tot.src = ew + K;
            tot.mean = dm + o_em + g; tot.sd = dm + o_es + g; tot.q = dm + o_eq + (long long)g * Q;
            tot.counts = d_counts.as<int32_t>() + 2 * g;
            const int si = (int)sets.size();
            sets.push_back(comp);
            sets.push_back(tot);
            set_scratch.push_back(-1);
            set_scratch.push_back(-1);
            for (int k = 0; k < K; ++k) ctasks.push_back(make_int2(si, k));
            ctasks.push_back(make_int2(si + 1, 0));
            pix_off += P; ew_off += (long long)S * (K + 1); s_off += S; comp_off += K;
        }
        close();
    }
    if (etasks.size() > 0x7fffffff || ctasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");
    HIP_TRY(hipMalloc(&d_scratch.p, (size_t)scratch_len * sizeof(double)));
    for (size_t i = 0; i < items.size(); ++i) items[i].flux = d_scratch.as<double>() + item_scratch[i];
    for (size_t i = 0; i < sets.size(); ++i)
        if (set_scratch[i] >= 0) sets[i].src = d_scratch.as<double>() + set_scratch[i];

    DevBuf d_items, d_sets, d_etasks, d_ctasks;
    if (upload(d_items, items, st) || upload(d_sets, sets, st) || upload(d_etasks, etasks, st) || upload(d_ctasks, ctasks, st)) return -1;
    for (const Pass& ps : passes) {
        if (ps.etask1 > ps.etask0) {
            hipLaunchKernelGGL(k_post_eval, dim3((unsigned)(ps.etask1 - ps.etask0)), dim3(kEvalBlock),
                               (size_t)kEvalWaves * ps.region_doubles * sizeof(double), st, d_items.as<Item>(),
                               d_etasks.as<int2>() + ps.etask0, ps.region_doubles);
            HIP_TRY(hipGetLastError());
        }
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
    std::vector<int32_t> counts((size_t)n_groups * 2);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < n_groups; ++g) {
        if (n_used) n_used[g] = counts[2 * g];
        if (n_bad) n_bad[g] = counts[2 * g + 1];
    }
    return 0;
}
