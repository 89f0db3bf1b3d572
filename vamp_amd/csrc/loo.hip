// loo.hip -- Pareto-smoothed importance-sampling leave-one-out predictive density of ensemble chains
// (include/vamp_loo.h, libvamp_loo.so).  Definitions: the header, and DESIGN.md "PSIS-LOO: leave-one-out predictive
// density per pixel".
//
// The work is a list of items (group, pixel range), packed greedily into passes whose log-likelihood scratch fits
// scratch_bytes (chain_groups.hpp, which posterior.hip and predictive.hip share).  The scratch of an item is
// pixel-major, ll[p * S + s]: what predictive.hip measured as the faster orientation for a column stage that streams
// its column.  Two launches per pass, one at the end:
//   k_pointwise_ll   vamp_loo_pointwise: the evaluation this library shares with predictive.hip (pointwise_ll.hpp), one
//                    workgroup per (item, 64 samples), pixel-major.
//   k_loo_transpose  vamp_loo_from_loglik: one workgroup per (item, 32 samples) brings the caller's sample-major matrix
//                    into the same scratch layout through 32 x 32 tiles in LDS.
//   k_loo_column     one workgroup of 1024 threads per column (a pixel's l over the samples); a thread holds its at most
//                    16 entries in registers.  The M <= 384 largest log ratios are found without sorting the column: a
//                    bisection over the 64 bits of the order-preserving integer image of the doubles, then over the 14
//                    bits of the sample index among the values tied at the threshold -- the counts are integers, so no
//                    order enters.  The tail is compacted into LDS and bitonic-sorted on (value, index); the Zhang-
//                    Stephens grid of log1p is spread over the workgroup, 16 threads per theta_j, each partial sum and
//                    each sum of partials in a fixed order; a thread finds the smoothed weight of a tail entry it holds
//                    by binary search of the sorted tail.  Every floating-point sum over the samples is a per-thread
//                    fold in sample order and a block reduction of fixed order, so a column's result depends neither
//                    on the pass it was packed into nor on the entry point it came through.
//   k_loo_totals     one thread per group: the group's sums over its per-pixel values, in pixel order.
// No kernel asks for more than 64 KiB of LDS.  Everything is fp64.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_loo.h"
#include "chain_groups.hpp"
#include "lane_group.hpp"
#include "pointwise_ll.hpp"
#include "side_call.hpp"
#include "voigt_math.hpp"

#define VAMP_LOO_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace vamp::side;

constexpr bool kNarrow = true;              // a 16-lane group may own a sample: predictive.hip's measurement
constexpr int kColBlock = 1024;            // one size for every column: the reduction order must not depend on the pass
constexpr int kColWaves = kColBlock / 64;
constexpr int kColPerThread = VAMP_LOO_MAX_SAMPLES / kColBlock;
constexpr int kMaxTail = 384;              // M at n = VAMP_LOO_MAX_SAMPLES
constexpr int kSortSlots = 512;            // the bitonic sort's size: a power of two >= kMaxTail
constexpr int kMaxFit = 49;                // m = 30 + floor(sqrt(M)) at M = kMaxTail
constexpr int kFitLanes = 16;              // threads that share one theta_j of the grid
constexpr int kFitStride = kFitLanes + 1;  // their partial sums, padded: one thread per j reads a row
constexpr int kIndexBits = 14;             // sample index < 2^14
constexpr int kTile = 32;                  // the transpose's tile
constexpr int kTransBlock = 256;
constexpr int kTotBlock = 64;
constexpr double kHighKhat = 0.7;          // Vehtari, Gelman & Gabry (2017)

static_assert(kColPerThread * kColBlock == VAMP_LOO_MAX_SAMPLES && kColPerThread <= 32, "a thread's entries are a bit mask");
static_assert((1 << kIndexBits) == VAMP_LOO_MAX_SAMPLES, "the bisection over the sample index covers every index");
static_assert(kMaxTail * kMaxTail >= 9 * VAMP_LOO_MAX_SAMPLES && (kMaxTail - 1) * (kMaxTail - 1) < 9 * VAMP_LOO_MAX_SAMPLES &&
                  kMaxTail <= (VAMP_LOO_MAX_SAMPLES + 4) / 5 && kMaxTail <= kSortSlots && kSortSlots <= kColBlock,
              "the longest tail fits the sort");
static_assert((kMaxFit - 30) * (kMaxFit - 30) <= kMaxTail && (kMaxFit - 29) * (kMaxFit - 29) > kMaxTail &&
                  kMaxFit * kFitLanes <= kColBlock,
              "the grid of the fit fits the workgroup");

constexpr size_t kColumnLds = sizeof(double) * (kColBlock + kSortSlots + kMaxTail + kMaxFit * kFitStride + 2 * kMaxFit) +
                              sizeof(int) * (kSortSlots + 2 * kColWaves + 1);
static_assert(VAMP_LOO_MAX_COMPONENTS <= kEvalMaxComponents && kColumnLds <= 64 * 1024 && sizeof(double) * kTile * (kTile + 1) <= 64 * 1024,
              "a launch that asks for more than 64 KiB of LDS needs side::raise_lds_limit");

struct Matrix {                    // one (group, pixel range) of vamp_loo_from_loglik
    const double* src;             // the range's first column in the caller's [S][P] matrix (device)
    double* ll;                    // the item's scratch, [np][S]
    int S, P, np;
};

struct ColSet {                    // the columns of an item
    const double* src;             // l of (column c, sample s) = src[c * S + s]
    const uint8_t* bad;
    double* elpd;                  // [c]
    double* ploo;                  // [c]
    double* khat;                  // [c]
    double* lppd;                  // [c]
    int32_t* counts;               // {n_used, n_bad} of the group (written by column 0), or NULL
    int S;
};

struct Totals {                    // a group's per-pixel values
    const double* elpd;
    const double* ploo;
    const double* khat;
    int P;
};

// task: (item, first of kTile samples).  A tile is read along the pixels and written along the samples.
__global__ __launch_bounds__(kTransBlock) void k_loo_transpose(const Matrix* __restrict__ mats, const int2* __restrict__ tasks) {
    __shared__ double tile[kTile][kTile + 1];
    const int2 task = tasks[blockIdx.x];
    const Matrix A = mats[task.x];
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    constexpr int kRows = kTransBlock / kTile;
    for (int p0 = 0; p0 < A.np; p0 += kTile) {
        for (int r = ty; r < kTile; r += kRows) {
            const int s = task.y + r, p = p0 + tx;
            if (s < A.S && p < A.np) tile[r][tx] = A.src[(long long)s * A.P + p];
        }
        __syncthreads();
        for (int r = ty; r < kTile; r += kRows) {
            const int p = p0 + r, s = task.y + tx;
            if (s < A.S && p < A.np) A.ll[(long long)p * A.S + s] = tile[tx][r];
        }
        __syncthreads();
    }
}

// the tail length M of n good samples: min(ceil(n / 5), smallest m3 with m3^2 >= 9 n), in integers
__device__ __forceinline__ int tail_length(int n) {
    int m3 = (int)sqrt(9.0 * (double)n);
    while (m3 * m3 < 9 * n) ++m3;
    while (m3 > 0 && (m3 - 1) * (m3 - 1) >= 9 * n) --m3;
    return min((n + 4) / 5, m3);
}

// the unsigned integer whose order is the order of the doubles (no NaN among them)
__device__ __forceinline__ unsigned long long order_key(double v) {
    const long long b = __double_as_longlong(v);
    return b < 0 ? ~(unsigned long long)b : (unsigned long long)b | 0x8000000000000000ull;
}

// sum of an integer over the workgroup: a butterfly in the wavefront, then the wavefronts' sums through LDS.  buf:
// 2 * kColWaves ints used alternately, so that one barrier per call is enough; round: the calls so far (uniform)
__device__ __forceinline__ int block_count(int c, int* buf, int& round) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    int* b = buf + (round & 1) * kColWaves;
    if ((threadIdx.x & 63) == 0) b[threadIdx.x >> 6] = c;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kColWaves; ++w) total += b[w];
    ++round;
    return total;
}

__global__ __launch_bounds__(kColBlock) void k_loo_column(const ColSet* __restrict__ sets, const int2* __restrict__ tasks) {
    __shared__ double red[kColBlock];
    __shared__ double sv[kSortSlots];                  // the tail, ascending by (value, index)
    __shared__ int si[kSortSlots];
    __shared__ double xs[kMaxTail];                    // x_i; later the smoothed log weights
    __shared__ double part[kMaxFit * kFitStride];
    __shared__ double th[kMaxFit], lj[kMaxFit];
    __shared__ int cnt[2 * kColWaves];
    __shared__ int fill;
    const int2 task = tasks[blockIdx.x];
    const ColSet C = sets[task.x];
    const int c = task.y, tid = threadIdx.x;
    const double* src = C.src + (long long)c * C.S;

    double v[kColPerThread];
    unsigned have = 0u;                                // the thread's entries that are good samples
    int nb = 0, nn = 0, nf = 0;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j) {
        const int i = tid + j * kColBlock;
        v[j] = 0.0;
        if (i < C.S) {
            if (C.bad[i]) ++nb;
            else {
                v[j] = src[i];
                have |= 1u << j;
                if (isnan(v[j])) ++nn;
                if (!isfinite(v[j])) ++nf;
            }
        }
    }
    int round = 0;                                     // of block_count
    const int n_bad = block_count(nb, cnt, round);
    const int n_nan = block_count(nn, cnt, round);
    const int n_notfinite = block_count(nf, cnt, round);
    const int n = C.S - n_bad;

    // lppd, as k_pred_column forms it
    double fold = -INFINITY;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j)
        if (have >> j & 1u) fold = fmax(fold, v[j]);
    const double lmax = vamp::block_max<kColBlock>(fold, red);
    fold = 0.0;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j)
        if (have >> j & 1u) fold += exp(v[j] - lmax);
    const double sum_exp = vamp::block_sum<kColBlock>(fold, red);
    const double lppd = (n == 0 || n_nan > 0) ? NAN : lmax + log(sum_exp / (double)n);
    if (tid == 0 && C.counts && c == 0) { C.counts[0] = n; C.counts[1] = n_bad; }
    if (n == 0 || n_notfinite > 0) {                   // (uniform)
        if (tid == 0) { C.lppd[c] = lppd; C.elpd[c] = NAN; C.ploo[c] = NAN; C.khat[c] = NAN; }
        return;
    }

    // log ratios
    double lw[kColPerThread];
    fold = -INFINITY;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j) {
        lw[j] = -v[j];
        if (have >> j & 1u) fold = fmax(fold, lw[j]);
    }
    const double rmax = vamp::block_max<kColBlock>(fold, red);
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j) lw[j] = lw[j] - rmax;

    const int M = tail_length(n);
    double khat = INFINITY;
    if (M >= 5) {                                      // (uniform, as every branch on a reduced value below)
        // 1. the M-th largest value: the largest T with #{key >= T} >= M, one key bit per round (two bits per round, three
        //    thresholds counted at once, gave the same bits and was 1 % slower: profiles/loo_bench.txt)
        unsigned long long T = 0ull;
        for (int b = 63; b >= 0; --b) {
            const unsigned long long cand = T | (1ull << b);
            int k = 0;
#pragma unroll
            for (int j = 0; j < kColPerThread; ++j) k += ((have >> j & 1u) && order_key(lw[j]) >= cand) ? 1 : 0;
            if (block_count(k, cnt, round) >= M) T = cand;
        }
        int k_gt = 0, k_eq = 0;
#pragma unroll
        for (int j = 0; j < kColPerThread; ++j)
            if (have >> j & 1u) {
                const unsigned long long key = order_key(lw[j]);
                k_gt += key > T ? 1 : 0;
                k_eq += key == T ? 1 : 0;
            }
        const int need = M - block_count(k_gt, cnt, round);            // of the values tied at T: those of the largest indices
        const int n_eq = block_count(k_eq, cnt, round);
        int first = 0;                                                 // the smallest index of a tied value in the tail
        if (n_eq > need)
            for (int b = kIndexBits - 1; b >= 0; --b) {
                const int cand = first | (1 << b);
                int k = 0;
#pragma unroll
                for (int j = 0; j < kColPerThread; ++j)
                    k += ((have >> j & 1u) && order_key(lw[j]) == T && tid + j * kColBlock >= cand) ? 1 : 0;
                if (block_count(k, cnt, round) >= need) first = cand;
            }
        unsigned tail = 0u;
        fold = -INFINITY;
#pragma unroll
        for (int j = 0; j < kColPerThread; ++j)
            if (have >> j & 1u) {
                const unsigned long long key = order_key(lw[j]);
                if (key > T || (key == T && tid + j * kColBlock >= first)) tail |= 1u << j;
                else fold = fmax(fold, lw[j]);
            }
        const double cutoff = vamp::block_max<kColBlock>(fold, red);

        // 2. the tail into LDS, in any order, and sorted there: (value, index) has no ties
        int slots = 8;
        while (slots < M) slots <<= 1;
        if (tid == 0) fill = 0;
        if (tid < slots) { sv[tid] = INFINITY; si[tid] = INT_MAX; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kColPerThread; ++j)
            if (tail >> j & 1u) {
                const int slot = atomicAdd(&fill, 1);
                if (slot < slots) { sv[slot] = lw[j]; si[slot] = tid + j * kColBlock; }
            }
        __syncthreads();
        for (int k = 2; k <= slots; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int p = tid ^ j;
                if (tid < slots && p > tid) {
                    const double a = sv[tid], b = sv[p];
                    const int ia = si[tid], ib = si[p];
                    const bool greater = a > b || (a == b && ia > ib);
                    if (greater == ((tid & k) == 0)) { sv[tid] = b; sv[p] = a; si[tid] = ib; si[p] = ia; }
                }
                __syncthreads();
            }

        // 3. the generalised Pareto fit of x_i = exp(r_tail,i) - exp(cutoff)
        const double exp_cut = exp(cutoff);
        if (tid < M) xs[tid] = exp(sv[tid]) - exp_cut;
        __syncthreads();
        const double xq = xs[(M + 2) / 4 - 1], x_last = xs[M - 1];
        if (sv[M - 1] > sv[0] && xq > 0.0) {
            const double dM = (double)M;
            int root = (int)sqrt(dM);
            while (root * root > M) --root;
            while ((root + 1) * (root + 1) <= M) ++root;
            const int m = 30 + root;
            if (tid < m) th[tid] = 1.0 / x_last + (1.0 - sqrt((double)m / ((double)(tid + 1) - 0.5))) / (3.0 * xq);
            __syncthreads();
            {
                const int j = tid / kFitLanes, t = tid - j * kFitLanes;
                if (j < m) {
                    const double theta = th[j];
                    double s = 0.0;
                    for (int i = t; i < M; i += kFitLanes) s += log1p(-theta * xs[i]);
                    part[j * kFitStride + t] = s;
                }
            }
            __syncthreads();
            if (tid < m) {
                double s = 0.0;
                for (int t = 0; t < kFitLanes; ++t) s += part[tid * kFitStride + t];
                const double kj = s / dM;
                lj[tid] = dM * (log(-th[tid] / kj) - kj - 1.0);
            }
            __syncthreads();
            if (tid < m) {
                const double mine = lj[tid];
                double s = 0.0;
                for (int i = 0; i < m; ++i) s += exp(lj[i] - mine);
                part[tid * kFitStride] = th[tid] * (1.0 / s);
            }
            __syncthreads();
            double theta_hat = 0.0;
            for (int j = 0; j < m; ++j) theta_hat += part[j * kFitStride];
            const double k = vamp::block_sum<kColBlock>(tid < M ? log1p(-theta_hat * xs[tid]) : 0.0, red) / dM;
            const double sigma = -k / theta_hat;
            khat = (k * dM + 5.0) / (dM + 10.0);

            // 4. the smoothed tail, each weight to the thread that holds its sample
            if (isfinite(khat)) {
                if (tid < M) {
                    const double p = ((double)(tid + 1) - 0.5) / dM;
                    xs[tid] = log(sigma * expm1(-khat * log1p(-p)) / khat + exp_cut);
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < kColPerThread; ++j)
                    if (tail >> j & 1u) {
                        const double val = lw[j];
                        const int idx = tid + j * kColBlock;
                        int lo = 0, hi = M - 1;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            const double a = sv[mid];
                            if (a < val || (a == val && si[mid] < idx)) lo = mid + 1;
                            else hi = mid;
                        }
                        lw[j] = xs[lo];
                    }
            }
        }
    }

    // truncate at 0, normalise, and the leave-one-out density
    fold = -INFINITY;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j) {
        lw[j] = lw[j] > 0.0 ? 0.0 : lw[j];
        if (have >> j & 1u) fold = fmax(fold, lw[j]);
    }
    const double wmax = vamp::block_max<kColBlock>(fold, red);
    fold = 0.0;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j)
        if (have >> j & 1u) fold += exp(lw[j] - wmax);
    const double lse = wmax + log(vamp::block_sum<kColBlock>(fold, red));
    fold = -INFINITY;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j)
        if (have >> j & 1u) {                          // (l read again: cheaper than 32 registers held through the selection)
            lw[j] = __builtin_nontemporal_load(src + tid + j * kColBlock) + (lw[j] - lse);
            fold = fmax(fold, lw[j]);
        }
    const double vmax = vamp::block_max<kColBlock>(fold, red);
    fold = 0.0;
#pragma unroll
    for (int j = 0; j < kColPerThread; ++j)
        if (have >> j & 1u) fold += exp(lw[j] - vmax);
    const double elpd = vmax + log(vamp::block_sum<kColBlock>(fold, red));
    if (tid == 0) { C.lppd[c] = lppd; C.elpd[c] = elpd; C.ploo[c] = lppd - elpd; C.khat[c] = khat; }
}

// out: [3][G] doubles (elpd_loo, elpd_loo_se, p_loo); n_high_k: [G]
__global__ __launch_bounds__(kTotBlock) void k_loo_totals(const Totals* __restrict__ tot, int G, double* __restrict__ out,
                                                          int32_t* __restrict__ n_high_k) {
    const int g = blockIdx.x * kTotBlock + threadIdx.x;
    if (g >= G) return;
    const Totals T = tot[g];
    double elpd = 0.0, pl = 0.0;
    int high = 0;
    for (int p = 0; p < T.P; ++p) {
        elpd += T.elpd[p];
        pl += T.ploo[p];
        high += T.khat[p] > kHighKhat ? 1 : 0;
    }
    const double mean = elpd / (double)T.P;
    double ss = 0.0;
    for (int p = 0; p < T.P; ++p) {
        const double d = T.elpd[p] - mean;
        ss = fma(d, d, ss);
    }
    out[g] = elpd;
    out[G + g] = T.P < 2 ? NAN : sqrt((double)T.P * (ss / (double)(T.P - 1)));
    out[2 * G + g] = pl;
    n_high_k[g] = high;
}

struct Pass {
    size_t etask0 = 0, etask1 = 0;     // its k_pointwise_ll or k_loo_transpose workgroups
    size_t ctask0 = 0, ctask1 = 0;     // its k_loo_column workgroups
    size_t range0 = 0, range1 = 0;     // its ranges of the plan
    int region_doubles = 0;            // LDS of a wavefront of k_pointwise_ll
    long long used = 0;                // doubles of the scratch it fills
};

struct Outputs {                   // the caller's arrays
    double *elpd_pix, *ploo_pix, *khat, *lppd, *elpd, *se, *ploo;
    int32_t *n_high_k, *n_used, *n_bad;
};

// What both entry points share once their scratch is planned: the column sets and tasks of every pass (prepare), the
// column launch of a pass, and the totals and the copies back (finish).  The per-pixel and per-group results live in
// d_out: elpd | p_loo | khat | lppd (tot_pix each) | group sums (3 G).
struct Frame {
    DevBuf d_out, d_counts, d_sets, d_totals, d_ctasks;
    long long tot_pix = 0;
    int G = 0;
    double* out() const { return d_out.as<double>(); }
};

int prepare(Frame& F, const std::string& fn, const PassPlan& plan, const std::vector<int>& S, const int32_t* n_pix, int G,
            long long tot_pix, double* scratch, const uint8_t* d_bad, std::vector<Pass>& passes, hipStream_t st) {
    F.tot_pix = tot_pix;
    F.G = G;
    HIP_TRY(hipMalloc(&F.d_out.p, (size_t)(4 * tot_pix + 3ll * G) * sizeof(double)));
    HIP_TRY(hipMalloc(&F.d_counts.p, (size_t)G * 3 * sizeof(int32_t)));          // {n_used, n_bad} per group, then n_high_k
    double* o = F.out();
    std::vector<ColSet> sets;
    std::vector<Totals> totals;
    std::vector<int2> ctasks;
    passes.assign(plan.first.size(), Pass{});
    long long pix_off = 0, s_off = 0;
    for (size_t i = 0; i < plan.ranges.size(); ++i) {
        const Range& r = plan.ranges[i];
        const int g = r.group, P = n_pix[g];
        Pass& ps = passes[r.pass];
        if (r.offset == 0) { ps.ctask0 = ctasks.size(); ps.range0 = i; }
        ColSet cs;
        cs.src = scratch + r.offset;
        cs.bad = d_bad + s_off;
        cs.elpd = o + pix_off + r.p0;
        cs.ploo = o + tot_pix + pix_off + r.p0;
        cs.khat = o + 2 * tot_pix + pix_off + r.p0;
        cs.lppd = o + 3 * tot_pix + pix_off + r.p0;
        cs.counts = r.p0 == 0 ? F.d_counts.as<int32_t>() + 2 * g : nullptr;
        cs.S = S[g];
        for (int c = 0; c < r.np; ++c) ctasks.push_back(make_int2((int)i, c));
        sets.push_back(cs);
        ps.ctask1 = ctasks.size();
        ps.range1 = i + 1;
        ps.used = r.offset + (long long)r.np * S[g];
        if (r.p0 + r.np == P) {
            Totals t;
            t.elpd = o + pix_off; t.ploo = o + tot_pix + pix_off; t.khat = o + 2 * tot_pix + pix_off; t.P = P;
            totals.push_back(t);
            pix_off += P; s_off += S[g];
        }
    }
    if (ctasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");
    if (upload(F.d_sets, sets, st) || upload(F.d_totals, totals, st) || upload(F.d_ctasks, ctasks, st)) return -1;
    return 0;
}

int launch_columns(const Frame& F, const Pass& ps, hipStream_t st) {
    hipLaunchKernelGGL(k_loo_column, dim3((unsigned)(ps.ctask1 - ps.ctask0)), dim3(kColBlock), 0, st, F.d_sets.as<ColSet>(),
                       F.d_ctasks.as<int2>() + ps.ctask0);
    HIP_TRY(hipGetLastError());
    return 0;
}

int finish(const Frame& F, const Outputs& o, hipStream_t st) {
    const long long tp = F.tot_pix, G = F.G, sz = sizeof(double);
    double* d = F.out();
    int32_t* d_high = F.d_counts.as<int32_t>() + 2 * G;
    hipLaunchKernelGGL(k_loo_totals, dim3((unsigned)((G + kTotBlock - 1) / kTotBlock)), dim3(kTotBlock), 0, st,
                       F.d_totals.as<Totals>(), (int)G, d + 4 * tp, d_high);
    HIP_TRY(hipGetLastError());
    if (fetch(o.elpd_pix, d, tp * sz, st) || fetch(o.ploo_pix, d + tp, tp * sz, st) || fetch(o.khat, d + 2 * tp, tp * sz, st) ||
        fetch(o.lppd, d + 3 * tp, tp * sz, st) || fetch(o.elpd, d + 4 * tp, G * sz, st) || fetch(o.se, d + 4 * tp + G, G * sz, st) ||
        fetch(o.ploo, d + 4 * tp + 2 * G, G * sz, st) || fetch(o.n_high_k, d_high, G * (long long)sizeof(int32_t), st))
        return -1;
    return fetch_counts(F.d_counts, (int)G, o.n_used, o.n_bad, st);
}

}  // namespace

VAMP_LOO_API int vamp_loo_version(void) { return VAMP_LOO_ABI_VERSION; }

VAMP_LOO_API const char* vamp_loo_last_error(void) { return g_err.c_str(); }

VAMP_LOO_API int vamp_loo_pointwise(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                                    const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                                    const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                                    const int32_t* n_keep, const int32_t* walkers, int64_t scratch_bytes, double* elpd_loo_pix,
                                    double* p_loo_pix, double* khat, double* lppd, double* elpd_loo, double* elpd_loo_se,
                                    double* p_loo, int32_t* n_high_k, int32_t* n_used, int32_t* n_bad, double* const* ll) {
    g_err.clear();
    const std::string fn = "vamp_loo_pointwise: ";
    if (n_groups <= 0) return fail(fn + "n_groups must be positive");
    if (!x || !flux || !noise || !n_pix || !n_comp || !mode || !sample_sd || !base || !ld || !n_keep || !walkers)
        return fail(fn + "NULL argument");
    ChainGroups cg;
    const std::string err = check_chain_groups(fn, n_groups, x, n_pix, n_comp, mode, sample_sd, base, ld, n_keep, walkers, scratch_bytes,
                                               VAMP_LOO_MAX_SAMPLES, VAMP_LOO_MAX_COMPONENTS,
                                               "subsample in time: ld * step, ceil(n_keep / step)", cg);
    if (!err.empty()) return fail(err);
    const long long tot_pix = cg.tot_pix, tot_s = cg.tot_s;
    long long tot_noise = 0;
    const std::string data_err = check_chain_data(fn, n_groups, flux, noise, n_pix, sample_sd, tot_noise);
    if (!data_err.empty()) return fail(data_err);
    if (tot_pix > (1LL << 30)) return fail(fn + "too many outputs");
    bool want_ll = false;
    for (int g = 0; ll && g < n_groups; ++g) want_ll |= ll[g] != nullptr;

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

    // one buffer of doubles: abscissae | data | noise | ln noise
    DataOffsets in;
    const std::vector<double> h_in = pack_chain_data(n_groups, x, flux, noise, n_pix, tot_pix, tot_noise, in);
    DevBuf d_in, d_bad, d_scratch;
    if (upload(d_in, h_in, st)) return -1;
    HIP_TRY(hipMalloc(&d_bad.p, (size_t)tot_s));

    const PassPlan plan = plan_passes(cg.cap, cg.S, n_pix, n_groups);
    HIP_TRY(hipMalloc(&d_scratch.p, (size_t)plan.scratch_len * sizeof(double)));
    Frame F;
    std::vector<Pass> passes;
    if (prepare(F, fn, plan, cg.S, n_pix, n_groups, tot_pix, d_scratch.as<double>(), d_bad.as<uint8_t>(), passes, st)) return -1;

    std::vector<Item> items;
    std::vector<int2> etasks;
    build_eval(plan, cg, in, d_in.as<double>(), noise, n_pix, n_comp, mode, ld, walkers, dbase, kNarrow, d_scratch.as<double>(),
               d_bad.as<uint8_t>(), items, etasks, passes);
    if (etasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");
    std::vector<long long> group_s_off(n_groups, 0);     // of a group's flags in d_bad
    for (int g = 1; g < n_groups; ++g) group_s_off[g] = group_s_off[g - 1] + cg.S[g - 1];

    DevBuf d_items, d_etasks;
    if (upload(d_items, items, st) || upload(d_etasks, etasks, st)) return -1;
    std::vector<double> h_scratch;
    std::vector<uint8_t> h_bad;
    for (const Pass& ps : passes) {
        if (launch_eval<true>(ps, d_items, d_etasks, st)) return -1;
        if (launch_columns(F, ps, st)) return -1;
        if (want_ll) {
            // the pass's scratch back before the next pass overwrites it; a bad sample's row was never written
            h_scratch.resize((size_t)ps.used);
            h_bad.resize((size_t)tot_s);
            HIP_TRY(hipMemcpyAsync(h_scratch.data(), d_scratch.p, (size_t)ps.used * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(h_bad.data(), d_bad.p, (size_t)tot_s, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (size_t i = ps.range0; i < ps.range1; ++i) {
                const Range& r = plan.ranges[i];
                double* out = ll[r.group];
                if (!out) continue;
                const int S = cg.S[r.group], P = n_pix[r.group];
                const uint8_t* bad = h_bad.data() + group_s_off[r.group];
                const double* m = h_scratch.data() + r.offset;
                for (int s = 0; s < S; ++s)
                    for (int p = 0; p < r.np; ++p)
                        out[(long long)s * P + r.p0 + p] = bad[s] ? NAN : m[(long long)p * S + s];
            }
        }
    }
    const Outputs o{elpd_loo_pix, p_loo_pix, khat, lppd, elpd_loo, elpd_loo_se, p_loo, n_high_k, n_used, n_bad};
    return finish(F, o, st);
}

VAMP_LOO_API int vamp_loo_from_loglik(int device, void* hip_stream, int n_groups, const double* const* ll, int is_device,
                                      const int32_t* n_samples, const int32_t* n_pix, const uint8_t* const* skip,
                                      int64_t scratch_bytes, double* elpd_loo_pix, double* p_loo_pix, double* khat, double* lppd,
                                      double* elpd_loo, double* elpd_loo_se, double* p_loo, int32_t* n_high_k, int32_t* n_used,
                                      int32_t* n_bad) {
    g_err.clear();
    const std::string fn = "vamp_loo_from_loglik: ";
    if (n_groups <= 0) return fail(fn + "n_groups must be positive");
    if (!ll || !n_samples || !n_pix) return fail(fn + "NULL argument");
    if (scratch_bytes < 0) return fail(fn + "scratch_bytes must not be negative");
    std::vector<int> S(n_groups);
    long long tot_pix = 0, tot_s = 0;
    int s_max = 0;
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (!ll[g]) return fail(at + "NULL log-likelihood matrix");
        if (n_pix[g] <= 0) return fail(at + "n_pix must be positive");
        if (n_samples[g] <= 0) return fail(at + "n_samples must be positive");
        if (n_samples[g] > VAMP_LOO_MAX_SAMPLES)
            return fail(at + "n_samples = " + std::to_string(n_samples[g]) + " exceeds " + std::to_string(VAMP_LOO_MAX_SAMPLES) +
                        " (subsample the rows)");
        if (skip && skip[g])
            for (int s = 0; s < n_samples[g]; ++s)
                if (skip[g][s] > 1) return fail(at + "skip must be 0 or 1 at sample " + std::to_string(s));
        S[g] = n_samples[g];
        s_max = S[g] > s_max ? S[g] : s_max;
        tot_pix += n_pix[g];
        tot_s += S[g];
    }
    const long long cap = (scratch_bytes ? scratch_bytes : kDefaultScratch) / (long long)sizeof(double);
    if (cap < s_max)
        return fail(fn + "scratch_bytes = " + std::to_string(scratch_bytes) + " is less than one column of the largest group (" +
                    std::to_string((long long)s_max * (long long)sizeof(double)) + " bytes)");
    if (tot_pix > (1LL << 30)) return fail(fn + "too many outputs");

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    std::vector<const double*> dll(ll, ll + n_groups);
    DevBuf staging;
    if (!is_device) {
        std::vector<long long> len(n_groups);
        for (int g = 0; g < n_groups; ++g) len[g] = (long long)S[g] * n_pix[g];
        if (stage_chains(len, ll, st, staging, dll)) return -1;
    }
    std::vector<uint8_t> h_bad((size_t)tot_s, 0);
    {
        long long off = 0;
        for (int g = 0; g < n_groups; ++g) {
            if (skip && skip[g])
                for (int s = 0; s < S[g]; ++s) h_bad[off + s] = skip[g][s];
            off += S[g];
        }
    }
    DevBuf d_bad, d_scratch;
    if (upload(d_bad, h_bad, st)) return -1;

    const PassPlan plan = plan_passes(cap, S, n_pix, n_groups);
    HIP_TRY(hipMalloc(&d_scratch.p, (size_t)plan.scratch_len * sizeof(double)));
    Frame F;
    std::vector<Pass> passes;
    if (prepare(F, fn, plan, S, n_pix, n_groups, tot_pix, d_scratch.as<double>(), d_bad.as<uint8_t>(), passes, st)) return -1;

    std::vector<Matrix> mats;
    std::vector<int2> ttasks;
    for (const Range& r : plan.ranges) {
        Pass& ps = passes[r.pass];
        if (r.offset == 0) ps.etask0 = ttasks.size();
        Matrix m;
        m.src = dll[r.group] + r.p0;
        m.ll = d_scratch.as<double>() + r.offset;
        m.S = S[r.group]; m.P = n_pix[r.group]; m.np = r.np;
        const int ii = (int)mats.size();
        mats.push_back(m);
        for (int s0 = 0; s0 < m.S; s0 += kTile) ttasks.push_back(make_int2(ii, s0));
        ps.etask1 = ttasks.size();
    }
    if (ttasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");
    DevBuf d_mats, d_ttasks;
    if (upload(d_mats, mats, st) || upload(d_ttasks, ttasks, st)) return -1;
    for (const Pass& ps : passes) {
        hipLaunchKernelGGL(k_loo_transpose, dim3((unsigned)(ps.etask1 - ps.etask0)), dim3(kTransBlock), 0, st, d_mats.as<Matrix>(),
                           d_ttasks.as<int2>() + ps.etask0);
        HIP_TRY(hipGetLastError());
        if (launch_columns(F, ps, st)) return -1;
    }
    const Outputs o{elpd_loo_pix, p_loo_pix, khat, lppd, elpd_loo, elpd_loo_se, p_loo, n_high_k, n_used, n_bad};
    return finish(F, o, st);
}
