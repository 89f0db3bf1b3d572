// laplace.hip -- Laplace importance sampling: independent draws from a Gaussian proposal per region, the exact
// log-posterior at each, Pareto-smoothed importance ratios, and from them ln Z and the posterior's first two moments
// (include/vamp_laplace.h, libvamp_laplace.so).  Definitions: the header, and DESIGN.md section 16.
//
// A call is four launches on one stream:
//   k_lap_draw     one workgroup of four wavefronts per (group, 64 rows); row s < S is sample s, row S the centre.  The
//                  packed lower triangle of C and the centre are staged once in LDS.  A wavefront -- or, for short
//                  regions of few lines, a 16-lane group (lane_group.hpp) -- owns one row at a time: its lanes draw the
//                  pairs of z from Philox (draws.hpp), form theta = centre + C z in LDS, build the line records and
//                  near-axis tables, walk the pixels and reduce chi^2 by a butterfly of fixed order.  The evaluator is
//                  evidence.hip's eval_point restated: the two are unified when a refactoring can show identical code.
//   k_lap_weights  one workgroup of 1024 threads per group over the S ratios, a thread's at most 16 in registers:
//                  plain importance sampling, then loo.hip's column stage restated on r_s -- the M largest found by
//                  bisection over the order-preserving integer image, the tail bitonic-sorted in LDS, the Zhang-Stephens
//                  grid spread 16 threads per theta_j -- with -inf entries allowed.
//   k_lap_mean     one workgroup per (group, d): sum w~ theta_d
//   k_lap_cov      one workgroup per (group, d): row d of the weighted second central moments, e <= d, mirrored
// Every floating-point sum over the samples is a per-thread fold in sample order and a block reduction of fixed order.
// No kernel asks for more than 64 KiB of LDS.  Everything is fp64.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_laplace.h"
#include "draws.hpp"
#include "lane_group.hpp"
#include "side_call.hpp"
#include "voigt_math.hpp"

#define VAMP_LAPLACE_API extern "C" __attribute__((visibility("default")))

// whether a 16-lane group may own a row (tools/bench_laplace.py compares the two)
#ifndef VAMP_LAPLACE_NARROW
#define VAMP_LAPLACE_NARROW 1
#endif

namespace {

using namespace vamp::side;
using vamp::lds_fence;

constexpr int kBlock = 256;                // four wavefronts
constexpr int kWaves = kBlock / 64;
constexpr int kRec = 7;                    // doubles of a line record: centre, scale, damping, amplitude, pole, h y, ln prior
constexpr int kRows = 64;                  // rows per workgroup of k_lap_draw
constexpr int kMaxD = VAMP_LAPLACE_MAX_DIM;
constexpr double SQRT_LN2 = 0.83255461115769775635;
constexpr unsigned STREAM_NORMAL = 5;      // beside STREAM_MOVE / ACCEPT / SPLIT of draws.hpp and SWAP / PRIOR of evidence.hip

constexpr int kColBlock = 1024;            // the weights' workgroup: one size, so that the reduction order is one
constexpr int kColWaves = kColBlock / 64;
constexpr int kPerThread = VAMP_LAPLACE_MAX_SAMPLES / kColBlock;
constexpr int kMaxTail = 384;              // M at S = VAMP_LAPLACE_MAX_SAMPLES
constexpr int kSortSlots = 512;            // the bitonic sort's size: a power of two >= kMaxTail
constexpr int kMaxFit = 49;                // m = 30 + floor(sqrt(M)) at M = kMaxTail
constexpr int kFitLanes = 16;              // threads that share one theta_j of the grid
constexpr int kFitStride = kFitLanes + 1;
constexpr int kIndexBits = 14;             // sample index < 2^14
constexpr int kMomBlock = 256;

static_assert(kMaxD == 4 * VAMP_LAPLACE_MAX_COMPONENTS + 1, "D = q K + sd");
static_assert(kPerThread * kColBlock == VAMP_LAPLACE_MAX_SAMPLES && kPerThread <= 32, "a thread's entries are a bit mask");
static_assert((1 << kIndexBits) == VAMP_LAPLACE_MAX_SAMPLES, "the bisection over the sample index covers every index");
static_assert(kMaxTail * kMaxTail >= 9 * VAMP_LAPLACE_MAX_SAMPLES && (kMaxTail - 1) * (kMaxTail - 1) < 9 * VAMP_LAPLACE_MAX_SAMPLES &&
                  kMaxTail <= (VAMP_LAPLACE_MAX_SAMPLES + 4) / 5 && kMaxTail <= kSortSlots && kSortSlots <= kColBlock,
              "the longest tail fits the sort");
static_assert((kMaxFit - 30) * (kMaxFit - 30) <= kMaxTail && (kMaxFit - 29) * (kMaxFit - 29) > kMaxTail && kMaxFit * kFitLanes <= kColBlock,
              "the grid of the fit fits the workgroup");

struct Reg {                       // one group
    const double* x;               // device: abscissa, flux, 1 / noise (1 with the free sd)
    const double* f;
    const double* wt;
    const double* C;               // device: the packed lower triangle, C_de at d (d + 1) / 2 + e, then the centre [D]
    double* theta;                 // [S][D]
    double* z;                     // [S][D], or NULL
    double* lnp;                   // [S + 1]: entry S is the centre's
    double* lnq;                   // [S]
    double c_lo, c_hi, w_max, lp_c, lp_w, norm_const;
    double sum_ln_diag, half_d_ln2pi;
    int P, K, q, D, sd, lanes;     // lanes that own a row (vamp::group_lanes)
    int skip;                      // 1: no proposal (status 1)
    unsigned rid;                  // region_id
};

struct Grp {                       // what k_lap_weights reads and writes of one group
    const double* lnp;
    const double* lnq;
    double* lw;                    // [S]
    double* wn;                    // [S]: the normalised weights, for the moments
    int skip;
};

struct Mom {                       // what the moment kernels read and write of one group
    const double* theta;
    const double* wn;
    double* mean;                  // [D]
    double* sd;                    // [D]
    double* cov;                   // [D][D]
    int D;
};

// LDS of one row: z, theta, the line records, the near-axis tables
__host__ __device__ constexpr int slot_doubles(int D, int K, bool voigt) { return 2 * D + K * kRec + (voigt ? K * vamp::DTAB_N : 0); }
__host__ __device__ constexpr int head_doubles(int D) { return D * (D + 1) / 2 + D; }

constexpr int kNarrowD = 4 * vamp::kNarrowMaxK + 1;
constexpr int kNarrowLds = head_doubles(kNarrowD) + kWaves * (64 / vamp::kNarrowLanes) * slot_doubles(kNarrowD, vamp::kNarrowMaxK, true);
constexpr int kWideLds = head_doubles(kMaxD) + kWaves * slot_doubles(kMaxD, VAMP_LAPLACE_MAX_COMPONENTS, true);
constexpr size_t kColumnLds = sizeof(double) * (kColBlock + kSortSlots + kMaxTail + kMaxFit * kFitStride + 2 * kMaxFit) +
                              sizeof(int) * (kSortSlots + 2 * kColWaves + 1);
static_assert(sizeof(double) * kNarrowLds <= 64 * 1024 && sizeof(double) * kWideLds <= 64 * 1024 && kColumnLds <= 64 * 1024,
              "a launch that asks for more than 64 KiB of LDS needs side::raise_lds_limit");

__device__ __forceinline__ double xexp_logp(double v) {        // log(v exp(-v)), literally; -inf below 0
    if (!(v >= 0.0) || !isfinite(v)) return -INFINITY;
    return log(v * exp(-v));
}
__device__ __forceinline__ double uniform_logp(double v, double lo, double hi, double lp) { return (v >= lo && v <= hi) ? lp : -INFINITY; }

// ln pi and ln L of the parameters q[D] (LDS), by the `lanes` lanes of one group; gl: the lane's index in the group.
// Every lane of a wavefront calls it (the fences are the wavefront's); `valid` lanes take part.  All lanes of a group
// return the same values.  Outside the prior ln L is NaN, not evaluated.  (evidence.hip's eval_point, restated.)
__device__ __forceinline__ void eval_point(const Reg& R, const double* q, double* rec, double* dtab, int lanes, int gl, bool valid,
                                           double& lp_out, double& ll_out) {
    const bool voigt = R.q == 4;
    const int K = R.K;
    if (valid)
        for (int k = gl; k < K; k += lanes) {
            const double* th = q + R.q * k;
            const double a = th[0], c = th[1];
            double* r = rec + k * kRec;
            double l = xexp_logp(a) + uniform_logp(c, R.c_lo, R.c_hi, R.lp_c);
            r[0] = c;
            if (voigt) {
                const double Lw = th[2], G = th[3];
                l += uniform_logp(Lw, 0.0, R.w_max, R.lp_w) + uniform_logp(G, 0.0, R.w_max, R.lp_w);
                const double rG = 1.0 / G;
                const double y = (Lw * SQRT_LN2) * rG;
                r[1] = (2.0 * SQRT_LN2) * rG;
                r[2] = y;
                r[3] = a * y;                      // tau_k = A y sqrt(pi) H: the evaluator returns sqrt(pi) H
                r[4] = vamp::core_pole_factor(y);
                r[5] = vamp::core_hy(y);
                if (!(r[1] < INFINITY) || !(y < INFINITY)) l = -INFINITY;      // degenerate width: rejected
            } else {
                const double sg = th[2];
                l += uniform_logp(sg, 0.0, R.w_max, R.lp_w);
                r[1] = 1.0 / sg; r[2] = 0.0; r[3] = a; r[4] = 0.0; r[5] = 0.0;
                if (!(r[1] < INFINITY)) l = -INFINITY;
            }
            r[6] = l;
        }
    lds_fence();
    double lp = 0.0;
    if (valid) {
        for (int k = 0; k < K; ++k) lp += rec[k * kRec + 6];
        if (R.sd) lp += uniform_logp(q[R.D - 1], 0.0, 1.0, 0.0);
    }
    const bool good = valid && lp > -INFINITY;     // (false for NaN)
    if (good && voigt) vamp::fill_dtab<kRec>(dtab, rec, K, gl, lanes);
    lds_fence();
    double chi = 0.0;
    if (good)
        for (int p = gl; p < R.P; p += lanes) {
            const double xi = R.x[p];
            double tau = 0.0;
            for (int k = 0; k < K; ++k) tau += vamp::line_tau(voigt, xi, rec + k * kRec, dtab + k * vamp::DTAB_N);
            const double d = (R.f[p] - exp(-tau)) * R.wt[p];
            chi = fma(d, d, chi);
        }
    for (int o = lanes >> 1; o > 0; o >>= 1) chi += __shfl_xor(chi, o, 64);      // stays inside the aligned group
    lds_fence();                                   // the records are free for the next row
    double ll = NAN;
    if (good) {
        if (R.sd) {
            const double sd = q[R.D - 1], t = 1.0 / (sd * sd);
            ll = (double)R.P * 0.5 * log(t / (2.0 * vamp::PI)) - 0.5 * t * chi;
        } else {
            ll = -0.5 * chi + R.norm_const;
        }
        if (!isfinite(ll)) ll = -INFINITY;
    }
    lp_out = valid ? (good ? lp : -INFINITY) : 0.0;
    ll_out = ll;
}

// Dynamic LDS: the packed C, the centre, then kWaves * (64 / lanes) slots.
__global__ __launch_bounds__(kBlock) void k_lap_draw(const Reg* __restrict__ regs, int blocks_per_group, int S, unsigned long long seed) {
    extern __shared__ double lds[];
    const int g = blockIdx.x / blocks_per_group, jb = blockIdx.x - g * blocks_per_group;
    const Reg R = regs[g];
    const int D = R.D, tid = threadIdx.x;
    const int r0 = jb * kRows, r1 = min(r0 + kRows, S + 1);
    if (R.skip) {                                  // (uniform) no proposal: every per-sample value is NaN
        for (int i = tid; i < (r1 - r0) * D; i += kBlock) {
            const long long at = (long long)r0 * D + i;
            if (at < (long long)S * D) {
                R.theta[at] = NAN;
                if (R.z) R.z[at] = NAN;
            }
        }
        for (int row = r0 + tid; row < r1; row += kBlock) {
            R.lnp[row] = NAN;
            if (row < S) R.lnq[row] = NAN;
        }
        return;
    }
    const int wave = tid >> 6, lane = tid & 63;
    const int lanes = R.lanes;
    const vamp::LaneGroup lg = vamp::lane_group(lane, lanes);
    const int nsub = lg.nsub, sub = lg.sub, gl = lg.gl;
    const bool voigt = R.q == 4;
    const int nC = D * (D + 1) / 2;
    double* Cs = lds;
    double* cen = Cs + nC;
    double* zs = cen + D + (size_t)(wave * nsub + sub) * slot_doubles(D, R.K, voigt);
    double* q = zs + D;
    double* rec = q + D;
    double* dtab = rec + R.K * kRec;
    for (int i = tid; i < nC + D; i += kBlock) Cs[i] = R.C[i];
    __syncthreads();

    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    for (int rb = r0 + wave * nsub; rb < r1; rb += kWaves * nsub) {            // (uniform per wavefront)
        const int row = rb + sub;
        const bool valid = row < r1, is_sample = row < S;
        if (valid)
            for (int j = gl; 2 * j < D; j += lanes) {
                double za = 0.0, zb = 0.0;                                      // the centre's row: z = 0
                if (is_sample) {
                    const vamp::U4 r = vamp::philox4x32_10({(unsigned)row, (unsigned)j, STREAM_NORMAL, R.rid}, k0, k1);
                    const double u1 = 1.0 - vamp::u53(r.c0, r.c1), u2 = vamp::u53(r.c2, r.c3);
                    const double rho = sqrt(-2.0 * log(u1));
                    double sn, cs;
                    sincos((2.0 * vamp::PI) * u2, &sn, &cs);
                    za = rho * cs;
                    zb = rho * sn;
                }
                zs[2 * j] = za;
                if (2 * j + 1 < D) zs[2 * j + 1] = zb;
            }
        lds_fence();
        if (valid)
            for (int d = gl; d < D; d += lanes) {
                const double* Cd = Cs + d * (d + 1) / 2;
                double acc = 0.0;
                for (int e = 0; e <= d; ++e) acc = fma(Cd[e], zs[e], acc);
                const double th = cen[d] + acc;
                q[d] = th;
                if (is_sample) {
                    R.theta[(long long)row * D + d] = th;
                    if (R.z) R.z[(long long)row * D + d] = zs[d];
                }
            }
        lds_fence();
        double zz = 0.0;
        if (valid && is_sample)
            for (int d = 0; d < D; ++d) zz = fma(zs[d], zs[d], zz);
        double lp, ll;
        eval_point(R, q, rec, dtab, lanes, gl, valid, lp, ll);
        if (valid && gl == 0) {
            R.lnp[row] = (lp > -INFINITY && isfinite(ll)) ? lp + ll : -INFINITY;
            if (is_sample) R.lnq[row] = (-0.5 * zz - R.sum_ln_diag) - R.half_d_ln2pi;
        }
    }
}

// the tail length M of n samples: min(ceil(n / 5), smallest m3 with m3^2 >= 9 n), in integers
__device__ __forceinline__ int tail_length(int n) {
    int m3 = (int)sqrt(9.0 * (double)n);
    while (m3 * m3 < 9 * n) ++m3;
    while (m3 > 0 && (m3 - 1) * (m3 - 1) >= 9 * n) --m3;
    return min((n + 4) / 5, m3);
}

// the unsigned integer whose order is the order of the doubles (no NaN among them; -inf is the smallest)
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

// out: [6][G] doubles (lnZ, lnZ_se, lnZ_psis, khat, ess, lnp_centre); iout: [3][G] ints (n_out, status, moments wanted)
__global__ __launch_bounds__(kColBlock) void k_lap_weights(const Grp* __restrict__ grps, int G, int S, double* __restrict__ out,
                                                           int32_t* __restrict__ iout) {
    __shared__ double red[kColBlock];
    __shared__ double sv[kSortSlots];                  // the tail, ascending by (value, index)
    __shared__ int si[kSortSlots];
    __shared__ double xs[kMaxTail];                    // x_i; later the smoothed log weights
    __shared__ double part[kMaxFit * kFitStride];
    __shared__ double th[kMaxFit], lj[kMaxFit];
    __shared__ int cnt[2 * kColWaves];
    __shared__ int fill;
    const int g = blockIdx.x, tid = threadIdx.x;
    const Grp A = grps[g];
    const double lnp_centre = A.skip ? NAN : A.lnp[S];
    const int status = A.skip ? 1 : (lnp_centre > -INFINITY ? 0 : 2);

    double lw[kPerThread];                             // r_s, then the log weights
    unsigned have = 0u;                                // the thread's entries that are samples
    int nf = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const int i = tid + j * kColBlock;
        lw[j] = -INFINITY;
        if (i < S) {
            have |= 1u << j;
            if (status == 0) {
                const double lp = A.lnp[i];
                if (lp > -INFINITY) { lw[j] = lp - A.lnq[i]; ++nf; }
            }
        }
    }
    int round = 0;                                     // of block_count
    const int n_fin = block_count(nf, cnt, round);
    if (status != 0 || n_fin == 0) {                   // (uniform)
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
            if (have >> j & 1u) { A.lw[tid + j * kColBlock] = NAN; A.wn[tid + j * kColBlock] = NAN; }
        if (tid == 0) {
            out[g] = status == 0 ? -INFINITY : NAN;
            for (int k = 1; k < 5; ++k) out[k * G + g] = NAN;
            out[5 * G + g] = lnp_centre;
            iout[g] = status == 0 ? S : 0;
            iout[G + g] = status;
            iout[2 * G + g] = 0;
        }
        return;
    }

    // plain importance sampling
    double fold = -INFINITY;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j)
        if (have >> j & 1u) fold = fmax(fold, lw[j]);
    const double rmax = vamp::block_max<kColBlock>(fold, red);
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) lw[j] = lw[j] - rmax;                 // (-inf stays -inf)
    fold = 0.0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j)
        if (have >> j & 1u) fold += exp(lw[j]);
    const double sum_w = vamp::block_sum<kColBlock>(fold, red);
    const double mean_w = sum_w / (double)S;
    fold = 0.0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j)
        if (have >> j & 1u) { const double d = exp(lw[j]) - mean_w; fold = fma(d, d, fold); }
    const double var_w = vamp::block_sum<kColBlock>(fold, red) / (double)(S - 1);
    const double lnZ = rmax + log(mean_w), lnZ_se = sqrt(var_w / (double)S) / mean_w;

    const int M = tail_length(S);
    double khat = INFINITY;
    if (M >= 5 && n_fin >= M + 1) {                    // (uniform, as every branch on a reduced value below)
        // 1. the M-th largest value: the largest T with #{key >= T} >= M, one key bit per round
        unsigned long long T = 0ull;
        for (int b = 63; b >= 0; --b) {
            const unsigned long long cand = T | (1ull << b);
            int k = 0;
#pragma unroll
            for (int j = 0; j < kPerThread; ++j) k += ((have >> j & 1u) && order_key(lw[j]) >= cand) ? 1 : 0;
            if (block_count(k, cnt, round) >= M) T = cand;
        }
        int k_gt = 0, k_eq = 0;
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
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
                for (int j = 0; j < kPerThread; ++j)
                    k += ((have >> j & 1u) && order_key(lw[j]) == T && tid + j * kColBlock >= cand) ? 1 : 0;
                if (block_count(k, cnt, round) >= need) first = cand;
            }
        unsigned tail = 0u;
        fold = -INFINITY;
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
            if (have >> j & 1u) {
                const unsigned long long key = order_key(lw[j]);
                if (key > T || (key == T && tid + j * kColBlock >= first)) tail |= 1u << j;
                else fold = fmax(fold, lw[j]);
            }
        const double cutoff = vamp::block_max<kColBlock>(fold, red);   // finite: at least M + 1 finite values

        // 2. the tail into LDS, in any order, and sorted there: (value, index) has no ties
        int slots = 8;
        while (slots < M) slots <<= 1;
        if (tid == 0) fill = 0;
        if (tid < slots) { sv[tid] = INFINITY; si[tid] = INT_MAX; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPerThread; ++j)
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
                for (int j = 0; j < kPerThread; ++j)
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

    // truncate at 0; the smoothed estimate, the normalised weights and their effective number
    fold = 0.0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        lw[j] = lw[j] > 0.0 ? 0.0 : lw[j];
        if (have >> j & 1u) {
            A.lw[tid + j * kColBlock] = lw[j];
            fold += exp(lw[j]);
        }
    }
    const double sum_e = vamp::block_sum<kColBlock>(fold, red);
    fold = 0.0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j)
        if (have >> j & 1u) {
            const double w = exp(lw[j]) / sum_e;
            A.wn[tid + j * kColBlock] = w;
            fold = fma(w, w, fold);
        }
    const double sum_w2 = vamp::block_sum<kColBlock>(fold, red);
    if (tid == 0) {
        out[g] = lnZ;
        out[G + g] = lnZ_se;
        out[2 * G + g] = rmax + log(sum_e / (double)S);
        out[3 * G + g] = khat;
        out[4 * G + g] = 1.0 / sum_w2;
        out[5 * G + g] = lnp_centre;
        iout[g] = S - n_fin;
        iout[G + g] = 0;
        iout[2 * G + g] = 1;
    }
}

// task: (group, d)
__global__ __launch_bounds__(kMomBlock) void k_lap_mean(const Mom* __restrict__ moms, const int2* __restrict__ tasks,
                                                        const int32_t* __restrict__ wanted, int S) {
    __shared__ double red[kMomBlock];
    const int2 task = tasks[blockIdx.x];
    const Mom A = moms[task.x];
    const int d = task.y, tid = threadIdx.x;
    if (!wanted[task.x]) {                             // (uniform)
        if (tid == 0) A.mean[d] = NAN;
        return;
    }
    double acc = 0.0;
    for (int s = tid; s < S; s += kMomBlock) acc = fma(A.wn[s], A.theta[(long long)s * A.D + d], acc);
    const double m = vamp::block_sum<kMomBlock>(acc, red);
    if (tid == 0) A.mean[d] = m;
}

__global__ __launch_bounds__(kMomBlock) void k_lap_cov(const Mom* __restrict__ moms, const int2* __restrict__ tasks,
                                                       const int32_t* __restrict__ wanted, int S) {
    __shared__ double red[kMomBlock];
    const int2 task = tasks[blockIdx.x];
    const Mom A = moms[task.x];
    const int D = A.D, d = task.y, tid = threadIdx.x;
    if (!wanted[task.x]) {                             // (uniform)
        if (tid <= d) { A.cov[d * D + tid] = NAN; A.cov[tid * D + d] = NAN; }
        if (tid == 0) A.sd[d] = NAN;
        return;
    }
    const double md = A.mean[d];
    for (int e = 0; e <= d; ++e) {
        const double me = A.mean[e];
        double acc = 0.0;
        for (int s = tid; s < S; s += kMomBlock) {
            const double* row = A.theta + (long long)s * D;
            acc = fma(A.wn[s] * (row[d] - md), row[e] - me, acc);
        }
        const double c = vamp::block_sum<kMomBlock>(acc, red);
        if (tid == 0) {
            A.cov[d * D + e] = c;
            A.cov[e * D + d] = c;
            if (e == d) A.sd[d] = sqrt(c);
        }
    }
}

// the checks of one group's data and its host-side record (pointers unset); `at` opens the message
int check_region(const std::string& at, const double* x, const double* flux, const double* noise, int P, int K, int mode, int sd,
                 const double* bounds, Reg& R) {
    if (!x || !flux) return fail(at + "NULL x or flux");
    if (P < 1) return fail(at + "n_pix must be positive");
    if (K < 1 || K > VAMP_LAPLACE_MAX_COMPONENTS)
        return fail(at + "n_comp = " + std::to_string(K) + " is outside 1 .. " + std::to_string(VAMP_LAPLACE_MAX_COMPONENTS));
    if (mode == 2) return fail(at + "mode 2 (NBZ3) is not supported: pass GAUSS3 (0) or VOIGT4 (1) parameters");
    if (mode != 0 && mode != 1) return fail(at + "mode must be 0 (GAUSS3) or 1 (VOIGT4)");
    if (sd != 0 && sd != 1) return fail(at + "sample_sd must be 0 or 1");
    if (!sd && !noise) return fail(at + "NULL noise");
    if (sd && noise) return fail(at + "noise must be NULL when sample_sd = 1");
    for (int p = 0; p < P; ++p) {
        if (!std::isfinite(x[p]) || !std::isfinite(flux[p])) return fail(at + "x or flux is not finite at pixel " + std::to_string(p));
        if (!sd && !(noise[p] > 0.0 && std::isfinite(noise[p]))) return fail(at + "noise must be positive and finite (pixel " + std::to_string(p) + ")");
    }
    if (P > 1) {
        const bool up = x[1] > x[0];
        for (int p = 1; p < P; ++p) {
            const double dx = x[p] - x[p - 1];
            if (dx == 0.0 || (dx > 0.0) != up) return fail(at + "x must be strictly monotonic (pixel " + std::to_string(p) + ")");
        }
    }
    R = Reg{};
    R.P = P; R.K = K; R.q = mode == 1 ? 4 : 3; R.sd = sd; R.D = R.q * K + sd;
    R.lanes = vamp::group_lanes(VAMP_LAPLACE_NARROW, P, K);
    if (bounds) {
        R.c_lo = bounds[0]; R.c_hi = bounds[1];
        R.w_max = mode == 0 ? bounds[2] : bounds[3];
    } else {
        R.c_lo = std::fmin(x[0], x[P - 1]); R.c_hi = std::fmax(x[0], x[P - 1]);
        const double sigma_max = (R.c_hi - R.c_lo) / 2.0;
        R.w_max = mode == 0 ? sigma_max : sigma_max * 2 * std::sqrt(2 * std::log(2.0));
    }
    if (!(R.c_hi > R.c_lo) || !(R.w_max > 0) || !std::isfinite(R.c_hi - R.c_lo) || !std::isfinite(R.w_max))
        return fail(at + "empty prior range" + (bounds ? "" : " (a region of one pixel needs bounds)"));
    R.lp_c = -std::log(R.c_hi - R.c_lo);
    R.lp_w = -std::log(R.w_max);
    double nc = 0.0;
    if (!sd) {
        for (int p = 0; p < P; ++p) nc += std::log(2.0 * M_PI * noise[p] * noise[p]);
        nc *= -0.5;
    }
    R.norm_const = nc;
    return 0;
}

// The proposal of one group into `packed` (the lower triangle row by row, then the centre) and the constants of ln q;
// returns whether there is a proposal (else status 1, and the group's slice of `packed` is zero)
bool pack_proposal(const double* centre, const double* chol, Reg& R, std::vector<double>& packed) {
    const int D = R.D;
    const size_t at = packed.size();
    packed.resize(at + (size_t)head_doubles(D), 0.0);
    bool ok = true;
    double sum = 0.0;
    for (int d = 0; d < D && ok; ++d) {
        for (int e = 0; e <= d && ok; ++e) ok = std::isfinite(chol[(size_t)d * D + e]);
        ok = ok && chol[(size_t)d * D + d] > 0.0 && std::isfinite(centre[d]);
    }
    if (!ok) return false;
    double* dst = packed.data() + at;
    for (int d = 0; d < D; ++d) {
        for (int e = 0; e <= d; ++e) *dst++ = chol[(size_t)d * D + e];
        sum += std::log(chol[(size_t)d * D + d]);
    }
    for (int d = 0; d < D; ++d) *dst++ = centre[d];
    R.sum_ln_diag = sum;
    R.half_d_ln2pi = 0.5 * (double)D * std::log(2.0 * M_PI);
    return true;
}

// x | flux | weights of the groups into one device buffer; sets the three pointers of every record
int upload_pixels(DevBuf& buf, std::vector<Reg>& regs, const double* const* x, const double* const* flux, const double* const* noise,
                  hipStream_t st, std::vector<double>& host) {
    long long tot = 0;
    for (const Reg& R : regs) tot += R.P;
    host.resize((size_t)tot * 3);
    HIP_TRY(hipMalloc(&buf.p, host.size() * sizeof(double)));
    long long o = 0;
    for (size_t g = 0; g < regs.size(); ++g) {
        Reg& R = regs[g];
        for (int p = 0; p < R.P; ++p) {
            host[o + p] = x[g][p];
            host[tot + o + p] = flux[g][p];
            host[2 * tot + o + p] = R.sd ? 1.0 : 1.0 / noise[g][p];
        }
        R.x = buf.as<double>() + o; R.f = R.x + tot; R.wt = R.x + 2 * tot;
        o += R.P;
    }
    HIP_TRY(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, st));
    return 0;
}

size_t draw_lds_bytes(const Reg& R) {
    return sizeof(double) * ((size_t)head_doubles(R.D) + (size_t)kWaves * (64 / R.lanes) * slot_doubles(R.D, R.K, R.q == 4));
}

}  // namespace

VAMP_LAPLACE_API int vamp_laplace_version(void) { return VAMP_LAPLACE_ABI_VERSION; }

VAMP_LAPLACE_API const char* vamp_laplace_last_error(void) { return g_err.c_str(); }

VAMP_LAPLACE_API int vamp_laplace_points(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                                         const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                                         const int32_t* sample_sd, const double* const* bounds, const int32_t* region_id,
                                         const double* const* centre, const double* const* chol, int n_samples, uint64_t seed,
                                         double* lnZ, double* lnZ_se, double* lnZ_psis, double* khat, double* ess, double* lnp_centre,
                                         int32_t* n_out, int32_t* status, double* mean, double* sd, double* cov, double* const* theta,
                                         double* const* z, int samples_are_device, double* const* lnp, double* const* lnq,
                                         double* const* lw) {
    g_err.clear();
    const std::string fn = "vamp_laplace_points: ";
    const int G = n_groups, S = n_samples;
    if (G <= 0) return fail(fn + "n_groups must be positive");
    if (!x || !flux || !noise || !n_pix || !n_comp || !mode || !sample_sd || !region_id || !centre || !chol) return fail(fn + "NULL argument");
    if (S < 2 || S > VAMP_LAPLACE_MAX_SAMPLES)
        return fail(fn + "n_samples = " + std::to_string(S) + " is outside 2 .. " + std::to_string(VAMP_LAPLACE_MAX_SAMPLES));
    if (samples_are_device != 0 && samples_are_device != 1) return fail(fn + "samples_are_device must be 0 or 1");
    std::vector<Reg> regs(G);
    std::vector<double> packed;
    std::vector<long long> head_off(G), vec_off(G), mat_off(G), own_theta(G, -1), own_z(G, -1);
    long long tot_vec = 0, tot_mat = 0, tot_theta = 0, n_own = 0;
    size_t lds_max = 0;
    for (int g = 0; g < G; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (check_region(at, x[g], flux[g], noise[g], n_pix[g], n_comp[g], mode[g], sample_sd[g], bounds ? bounds[g] : nullptr, regs[g])) return -1;
        if (region_id[g] < 0) return fail(at + "region_id is negative");
        if (!centre[g] || !chol[g]) return fail(at + "NULL centre or chol");
        Reg& R = regs[g];
        R.rid = (unsigned)region_id[g];
        head_off[g] = (long long)packed.size();
        R.skip = pack_proposal(centre[g], chol[g], R, packed) ? 0 : 1;
        vec_off[g] = tot_vec; mat_off[g] = tot_mat;
        tot_vec += R.D; tot_mat += (long long)R.D * R.D;
        tot_theta += (long long)S * R.D;
        // a buffer of the library's for every [S][D] block the caller does not hold on the device
        if (!(samples_are_device && theta && theta[g])) { own_theta[g] = n_own; n_own += (long long)S * R.D; }
        if (z && z[g] && !samples_are_device) { own_z[g] = n_own; n_own += (long long)S * R.D; }
        const size_t lds = draw_lds_bytes(R);
        lds_max = lds > lds_max ? lds : lds_max;
    }
    if (tot_theta > VAMP_LAPLACE_MAX_THETA_DOUBLES)
        return fail(fn + "more than " + std::to_string(VAMP_LAPLACE_MAX_THETA_DOUBLES) + " doubles of draws in one call: split it");
    const int blocks_per_group = (S + 1 + kRows - 1) / kRows;
    if ((long long)G * blocks_per_group > 0x7fffffffLL || tot_vec > 0x7fffffffLL) return fail(fn + "too many workgroups");

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    DevBuf d_pix, d_packed, d_regs, d_grps, d_moms, d_tasks, d_samples, d_rows, d_out, d_iout, d_mom_out;
    std::vector<double> pix;
    if (upload_pixels(d_pix, regs, x, flux, noise, st, pix)) return -1;
    if (upload(d_packed, packed, st)) return -1;
    if (n_own > 0) HIP_TRY(hipMalloc(&d_samples.p, (size_t)n_own * sizeof(double)));
    // per group: ln p [S + 1] | ln q [S] | lw [S] | w~ [S]
    const long long row_len = 4LL * S + 1;
    HIP_TRY(hipMalloc(&d_rows.p, (size_t)(G * row_len) * sizeof(double)));
    HIP_TRY(hipMalloc(&d_out.p, (size_t)G * 6 * sizeof(double)));
    HIP_TRY(hipMalloc(&d_iout.p, (size_t)G * 3 * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&d_mom_out.p, (size_t)(2 * tot_vec + tot_mat) * sizeof(double)));
    double* d_mean = d_mom_out.as<double>();
    double* d_sd = d_mean + tot_vec;
    double* d_cov = d_sd + tot_vec;

    std::vector<Grp> grps(G);
    std::vector<Mom> moms(G);
    std::vector<int2> tasks;
    for (int g = 0; g < G; ++g) {
        Reg& R = regs[g];
        double* rows = d_rows.as<double>() + g * row_len;
        R.C = d_packed.as<double>() + head_off[g];
        R.theta = own_theta[g] >= 0 ? d_samples.as<double>() + own_theta[g] : theta[g];
        R.z = (z && z[g]) ? (own_z[g] >= 0 ? d_samples.as<double>() + own_z[g] : z[g]) : nullptr;
        R.lnp = rows;
        R.lnq = rows + S + 1;
        grps[g] = Grp{R.lnp, R.lnq, rows + 2LL * S + 1, rows + 3LL * S + 1, R.skip};
        moms[g] = Mom{R.theta, grps[g].wn, d_mean + vec_off[g], d_sd + vec_off[g], d_cov + mat_off[g], R.D};
        for (int d = 0; d < R.D; ++d) tasks.push_back(make_int2(g, d));
    }
    if (upload(d_regs, regs, st) || upload(d_grps, grps, st) || upload(d_moms, moms, st) || upload(d_tasks, tasks, st)) return -1;

    hipLaunchKernelGGL(k_lap_draw, dim3((unsigned)(G * blocks_per_group)), dim3(kBlock), lds_max, st, d_regs.as<Reg>(), blocks_per_group, S,
                       (unsigned long long)seed);
    HIP_TRY(hipGetLastError());
    int32_t* d_wanted = d_iout.as<int32_t>() + 2 * G;
    hipLaunchKernelGGL(k_lap_weights, dim3((unsigned)G), dim3(kColBlock), 0, st, d_grps.as<Grp>(), G, S, d_out.as<double>(),
                       d_iout.as<int32_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lap_mean, dim3((unsigned)tasks.size()), dim3(kMomBlock), 0, st, d_moms.as<Mom>(), d_tasks.as<int2>(), d_wanted, S);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lap_cov, dim3((unsigned)tasks.size()), dim3(kMomBlock), 0, st, d_moms.as<Mom>(), d_tasks.as<int2>(), d_wanted, S);
    HIP_TRY(hipGetLastError());

    const long long sz = sizeof(double);
    double* o = d_out.as<double>();
    if (fetch(lnZ, o, G * sz, st) || fetch(lnZ_se, o + G, G * sz, st) || fetch(lnZ_psis, o + 2 * G, G * sz, st) ||
        fetch(khat, o + 3 * G, G * sz, st) || fetch(ess, o + 4 * G, G * sz, st) || fetch(lnp_centre, o + 5 * G, G * sz, st) ||
        fetch(n_out, d_iout.p, G * (long long)sizeof(int32_t), st) || fetch(status, d_iout.as<int32_t>() + G, G * (long long)sizeof(int32_t), st) ||
        fetch(mean, d_mean, tot_vec * sz, st) || fetch(sd, d_sd, tot_vec * sz, st) || fetch(cov, d_cov, tot_mat * sz, st))
        return -1;
    for (int g = 0; g < G; ++g) {
        const Reg& R = regs[g];
        const long long n = (long long)S * R.D * sz;
        if (!samples_are_device && ((theta && fetch(theta[g], R.theta, n, st)) || (z && fetch(z[g], R.z, n, st)))) return -1;
        if ((lnp && fetch(lnp[g], R.lnp, S * sz, st)) || (lnq && fetch(lnq[g], R.lnq, S * sz, st)) || (lw && fetch(lw[g], grps[g].lw, S * sz, st)))
            return -1;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
