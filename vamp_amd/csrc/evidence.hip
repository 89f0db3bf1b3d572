// evidence.hip -- log-evidence of every region from a ladder of tempered ensembles that exchange walkers
// (include/vamp_evid.h, libvamp_evid.so).  Definitions: DESIGN.md "Evidence".
//
// A run is a sequence of launches on one stream:
//   k_evid_init    one thread per (region, rung, walker): the start block, or a prior draw from Philox
//   k_evid_eval    ln L and ln pi of rows of parameters (the initial state; the test hook vamp_evid_lnlike)
//   k_evid_steps   one workgroup per (region, rung), the rung's walkers, ln L and ln pi in LDS, swap_every full
//                  stretch steps per launch.  A wavefront -- or, for short regions of few lines, a 16-lane group -- owns
//                  one mover at a time: the draws of draws.hpp, the proposal, its line records and near-axis tables
//                  staged by lane_group.hpp, the pixels walked a round of lanes at a time, chi^2 reduced
//                  by a butterfly of fixed order.  The lane width depends on (n_pix, K) only.
//   k_evid_swap    one thread per (region, pair, walker), after every launch of k_evid_steps but the last
//   k_evid_reduce  one workgroup per region: per-rung moments, the stepping-stone estimate with its block standard
//                  error, the trapezoid, the acceptance rates
// Everything is fp64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_evid.h"
#include "draws.hpp"
#include "lane_group.hpp"
#include "side_call.hpp"
#include "voigt_math.hpp"

#define VAMP_EVID_API extern "C" __attribute__((visibility("default")))

// whether a 16-lane group may own a mover (tools/bench_evid.py compares the two; profiles/evidence_bench.txt)
#ifndef VAMP_EVID_NARROW
#define VAMP_EVID_NARROW 1
#endif

namespace {

using namespace vamp::side;
using vamp::lds_fence;

constexpr int kBlock = 256;                // four wavefronts
constexpr int kWaves = kBlock / 64;
constexpr int kRec = 7;                    // doubles of a line record: centre, scale, damping, amplitude, pole, h y, ln prior
constexpr int kHead = 2;                   // doubles in front of the state of k_evid_steps
constexpr int kEvalRows = 64;              // rows of parameters per workgroup of k_evid_eval
constexpr int kMaxD = 4 * VAMP_EVID_MAX_COMPONENTS + 1;
constexpr double SQRT_LN2 = 0.83255461115769775635;
constexpr unsigned STREAM_SWAP = 3, STREAM_PRIOR = 4;      // beside STREAM_MOVE / ACCEPT / SPLIT of draws.hpp

struct Reg {                       // one region
    const double* x;               // device: abscissa, flux, 1 / noise (1 with the free sd)
    const double* f;
    const double* wt;
    double* chain;                 // the beta = 1 rung's kept chain [n_keep][W][D], or NULL
    double* chain_ll;              // [n_keep][W], or NULL
    double c_lo, c_hi, w_max, lp_c, lp_w, norm_const;
    long long theta_off;           // of the region's [T][W][D] state (k_evid_eval: of its rows)
    long long out_off;             // of the region's [T][W] ln L / ln pi
    int P, K, q, D, sd, lanes;     // lanes that own a mover (vamp::group_lanes)
    unsigned rid;                  // region_id
};

struct Sampler {                   // what draw_move reads (draws.hpp, "Sampler")
    long long W;
    int split_block;
    double a;
    unsigned long long seed;
    unsigned rid;
};
__host__ __device__ inline unsigned region_rng_id(const Sampler& S, int) { return S.rid; }

// LDS of one mover: the proposal, the line records, the near-axis tables
__host__ __device__ constexpr int slot_doubles(int D, int K, bool voigt) { return D + K * kRec + (voigt ? K * vamp::DTAB_N : 0); }

__device__ __forceinline__ double xexp_logp(double v) {        // log(v exp(-v)), literally; -inf below 0
    if (!(v >= 0.0) || !isfinite(v)) return -INFINITY;
    return log(v * exp(-v));
}
__device__ __forceinline__ double uniform_logp(double v, double lo, double hi, double lp) { return (v >= lo && v <= hi) ? lp : -INFINITY; }

// ln pi and ln L of the parameters q[D] (LDS), by the `lanes` lanes of one group; gl: the lane's index in the group.
// Every lane of a wavefront calls it (the fences are the wavefront's); `valid` lanes take part.  All lanes of a group
// return the same values.  Outside the prior ln L is NaN, not evaluated.
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
    lds_fence();                                   // the records are free for the next point
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

// ln of the tempered target; a point outside the prior or without a finite ln L is -inf
__device__ __forceinline__ double target(double lp, double ll, double beta) {
    if (!(lp > -INFINITY) || !isfinite(ll)) return -INFINITY;
    return lp + beta * ll;
}

__device__ __forceinline__ double u53_open(unsigned hi, unsigned lo) { return 1.0 - vamp::u53(hi, lo); }      // (0, 1]

// start == NULL entries: prior draws keyed by (seed, walker gid, parameter); counter {gid lo, d, STREAM_PRIOR, gid hi}
__global__ __launch_bounds__(kBlock) void k_evid_init(const Reg* __restrict__ regs, const double* const* __restrict__ start, int T,
                                                      int W, unsigned long long seed, double* __restrict__ X, long long total) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int w = (int)(i % W), j = (int)((i / W) % T), g = (int)(i / ((long long)W * T));
    const Reg R = regs[g];
    double* row = X + R.theta_off + ((long long)j * W + w) * R.D;
    const double* s = start[g];
    if (s) {
        for (int d = 0; d < R.D; ++d) row[d] = s[(long long)w * R.D + d];
        return;
    }
    const unsigned long long gid = ((unsigned long long)R.rid * T + j) * W + w;
    for (int d = 0; d < R.D; ++d) {
        const vamp::U4 r = vamp::philox4x32_10({(unsigned)gid, (unsigned)d, STREAM_PRIOR, (unsigned)(gid >> 32)}, (unsigned)seed,
                                               (unsigned)(seed >> 32));
        const double u1 = u53_open(r.c0, r.c1), u2 = u53_open(r.c2, r.c3);
        double v;
        if (R.sd && d == R.D - 1) v = u1;                                  // sd ~ U(0, 1)
        else {
            const int c = d % R.q;
            if (c == 0) v = -log(u1) - log(u2);                            // A ~ A exp(-A): the sum of two exponentials
            else if (c == 1) v = R.c_lo + (R.c_hi - R.c_lo) * vamp::u53(r.c0, r.c1);
            else v = R.w_max * u1;                                         // widths in (0, max]
        }
        row[d] = v;
    }
}

// rows of parameters: workgroup b serves rows [jb * rows_per_block, ...) of region b / blocks_per_region
__global__ __launch_bounds__(kBlock) void k_evid_eval(const Reg* __restrict__ regs, int blocks_per_region, int rows_per_block, int n_rows,
                                                      const double* __restrict__ theta, double* __restrict__ ll_out,
                                                      double* __restrict__ lp_out) {
    extern __shared__ double lds[];
    const int g = blockIdx.x / blocks_per_region, jb = blockIdx.x - g * blocks_per_region;
    const Reg R = regs[g];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lanes = R.lanes;
    const vamp::LaneGroup lg = vamp::lane_group(lane, lanes);
    const int nsub = lg.nsub, sub = lg.sub, gl = lg.gl;
    const bool voigt = R.q == 4;
    double* q = lds + (size_t)(wave * nsub + sub) * slot_doubles(R.D, R.K, voigt);
    double* rec = q + R.D;
    double* dtab = rec + R.K * kRec;
    const int r0 = jb * rows_per_block, r1 = min(r0 + rows_per_block, n_rows);
    for (int rb = r0 + wave * nsub; rb < r1; rb += kWaves * nsub) {          // (uniform per wavefront)
        const int row = rb + sub;
        const bool valid = row < r1;
        if (valid)
            for (int d = gl; d < R.D; d += lanes) q[d] = theta[R.theta_off + (long long)row * R.D + d];
        lds_fence();
        double lp, ll;
        eval_point(R, q, rec, dtab, lanes, gl, valid, lp, ll);
        if (valid && gl == 0) {
            ll_out[R.out_off + row] = ll;
            lp_out[R.out_off + row] = lp;
        }
    }
}

// Dynamic LDS: kHead doubles (the acceptance counter), W D + 2 W doubles of state, then kWaves * (64 / lanes) slots.
__global__ __launch_bounds__(kBlock) void k_evid_steps(const Reg* __restrict__ regs, const double* __restrict__ betas, int T, int W,
                                                       unsigned long long seed, double a, int step0, int n_steps, int burn, int n_keep,
                                                       double* __restrict__ Xg, double* __restrict__ llg, double* __restrict__ lpg,
                                                       double* __restrict__ trace, unsigned* __restrict__ nacc) {
    extern __shared__ double lds[];
    unsigned* acc_count = reinterpret_cast<unsigned*>(lds);       // (in the dynamic region: a static would shift its base off 16 bytes)
    const int g = blockIdx.x / T, j = blockIdx.x - g * T;
    const Reg R = regs[g];
    const double beta = betas[j];
    const int D = R.D, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int lanes = R.lanes;
    const vamp::LaneGroup lg = vamp::lane_group(lane, lanes);
    const int nsub = lg.nsub, sub = lg.sub, gl = lg.gl;
    const bool voigt = R.q == 4;
    double* X = lds + kHead;
    double* ll = X + (size_t)W * D;
    double* lp = ll + W;
    double* q = lp + W + (size_t)(wave * nsub + sub) * slot_doubles(D, R.K, voigt);
    double* rec = q + D;
    double* dtab = rec + R.K * kRec;
    double* Xrung = Xg + R.theta_off + (long long)j * W * D;
    const long long lrow = R.out_off + (long long)j * W;

    for (int i = tid; i < W * D; i += kBlock) X[i] = Xrung[i];
    for (int i = tid; i < W; i += kBlock) { ll[i] = llg[lrow + i]; lp[i] = lpg[lrow + i]; }
    if (tid == 0) *acc_count = 0u;
    __syncthreads();

    Sampler S;
    S.W = W; S.split_block = W; S.a = a; S.seed = seed; S.rid = R.rid * (unsigned)T + (unsigned)j;
    const int halfW = W >> 1, slots = kWaves * nsub;
    for (int s = 0; s < n_steps; ++s) {
        const unsigned step = (unsigned)(step0 + s);
        for (int half = 0; half < 2; ++half) {
            for (int ab = wave * nsub; ab < halfW; ab += slots) {                // (uniform per wavefront)
                const int a_loc = ab + sub;
                const bool valid = a_loc < halfW;
                const vamp::MoveDraw d = vamp::draw_move(S, step, half, 0, (long long)(valid ? a_loc : 0));
                const double* Xs = X + (size_t)d.ws * D;
                const double* Xc = X + (size_t)d.wc * D;
                if (valid)
                    for (int e = gl; e < D; e += lanes) q[e] = Xc[e] - (Xc[e] - Xs[e]) * d.z;      // q = c - (c - s) z
                lds_fence();
                double lp_q, ll_q;
                eval_point(R, q, rec, dtab, lanes, gl, valid, lp_q, ll_q);
                if (valid) {
                    const double diff = (double)(D - 1) * log(d.z) + target(lp_q, ll_q, beta) - target(lp[d.ws], ll[d.ws], beta);
                    if (d.logu < diff) {                                          // false for NaN
                        for (int e = gl; e < D; e += lanes) X[(size_t)d.ws * D + e] = q[e];
                        if (gl == 0) { ll[d.ws] = ll_q; lp[d.ws] = lp_q; atomicAdd(acc_count, 1u); }
                    }
                }
                lds_fence();
            }
            __syncthreads();
        }
        const int t = (int)step - burn;
        if (t >= 0) {
            double* tr = trace + (((long long)g * n_keep + t) * T + j) * W;
            for (int i = tid; i < W; i += kBlock) tr[i] = ll[i];
            if (j == T - 1) {
                if (R.chain)
                    for (int i = tid; i < W * D; i += kBlock) R.chain[(long long)t * W * D + i] = X[i];
                if (R.chain_ll)
                    for (int i = tid; i < W; i += kBlock) R.chain_ll[(long long)t * W + i] = ll[i];
            }
            __syncthreads();           // the next step's movers write what was just read
        }
    }
    for (int i = tid; i < W * D; i += kBlock) Xrung[i] = X[i];
    for (int i = tid; i < W; i += kBlock) { llg[lrow + i] = ll[i]; lpg[lrow + i] = lp[i]; }
    if (tid == 0) nacc[blockIdx.x] += *acc_count;
}

// swap n: pairs (j, j + 1), j = parity + 2 pr; u from counter {region_id, n, j << 8 | STREAM_SWAP, w}
__global__ __launch_bounds__(kBlock) void k_evid_swap(const Reg* __restrict__ regs, const double* __restrict__ betas, int T, int W,
                                                      unsigned long long seed, unsigned n, int n_pairs, double* __restrict__ Xg,
                                                      double* __restrict__ llg, double* __restrict__ lpg, unsigned* __restrict__ nswap,
                                                      uint8_t* __restrict__ swap_trace, int n_swaps, long long total) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int w = (int)(i % W), pr = (int)((i / W) % n_pairs), g = (int)(i / ((long long)W * n_pairs));
    const int j = (int)(n & 1u) + 2 * pr;
    const Reg R = regs[g];
    const long long i0 = R.out_off + (long long)j * W + w, i1 = i0 + W;
    const double l0 = llg[i0], l1 = llg[i1];
    const vamp::U4 r = vamp::philox4x32_10({R.rid, n, ((unsigned)j << 8) | STREAM_SWAP, (unsigned)w}, (unsigned)seed, (unsigned)(seed >> 32));
    const double u = vamp::u53(r.c0, r.c1);
    const double logu = u > 0.0 ? log(u) : -INFINITY;
    const bool yes = logu < (betas[j + 1] - betas[j]) * (l0 - l1);              // false for NaN
    if (swap_trace) swap_trace[(((long long)g * n_swaps + n) * (T - 1) + j) * W + w] = yes ? 1 : 0;
    if (!yes) return;
    double* a0 = Xg + R.theta_off + ((long long)j * W + w) * R.D;
    double* a1 = a0 + (long long)W * R.D;
    for (int d = 0; d < R.D; ++d) { const double v = a0[d]; a0[d] = a1[d]; a1[d] = v; }
    llg[i0] = l1; llg[i1] = l0;
    const double p0 = lpg[i0];
    lpg[i0] = lpg[i1]; lpg[i1] = p0;
    atomicAdd(&nswap[g * (T - 1) + j], 1u);
}

// log mean exp(db * ln L) over rung j's kept steps [t0, t1)
__device__ inline double log_mean_exp(const double* tr, int T, int W, int j, int t0, int t1, double db, double* red) {
    const int n = (t1 - t0) * W;
    double m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += kBlock) m = fmax(m, db * tr[((long long)(t0 + i / W) * T + j) * W + i % W]);
    m = vamp::block_max<kBlock>(m, red);
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) s += exp(db * tr[((long long)(t0 + i / W) * T + j) * W + i % W] - m);
    s = vamp::block_sum<kBlock>(s, red);
    return m + log(s / (double)n);
}

__global__ __launch_bounds__(kBlock) void k_evid_reduce(const double* __restrict__ betas, int T, int W, int n_keep, int n_steps, int n_swaps,
                                                        const double* __restrict__ trace, const unsigned* __restrict__ nacc,
                                                        const unsigned* __restrict__ nswap, double* __restrict__ lnZ,
                                                        double* __restrict__ lnZ_se, double* __restrict__ lnZ_ti,
                                                        double* __restrict__ mean_out, double* __restrict__ var_out,
                                                        double* __restrict__ move_acc, double* __restrict__ swap_acc) {
    __shared__ double red[kBlock];
    __shared__ double means[VAMP_EVID_MAX_TEMPS];
    const int g = blockIdx.x, tid = threadIdx.x;
    const double* tr = trace + (long long)g * n_keep * T * W;
    const int n = n_keep * W;
    for (int j = 0; j < T; ++j) {
        double s = 0.0;
        for (int i = tid; i < n; i += kBlock) s += tr[((long long)(i / W) * T + j) * W + i % W];
        const double mean = vamp::block_sum<kBlock>(s, red) / (double)n;
        s = 0.0;
        for (int i = tid; i < n; i += kBlock) { const double d = tr[((long long)(i / W) * T + j) * W + i % W] - mean; s = fma(d, d, s); }
        const double var = vamp::block_sum<kBlock>(s, red) / (double)n;
        if (tid == 0) {
            means[j] = mean;
            mean_out[g * T + j] = mean;
            var_out[g * T + j] = var;
            move_acc[g * T + j] = (double)nacc[g * T + j] / ((double)n_steps * (double)W);
        }
    }
    double z = 0.0;
    for (int j = 0; j + 1 < T; ++j) z += log_mean_exp(tr, T, W, j, 0, n_keep, betas[j + 1] - betas[j], red);
    double zb[VAMP_EVID_BLOCKS];
    if (n_keep >= VAMP_EVID_BLOCKS)
        for (int b = 0; b < VAMP_EVID_BLOCKS; ++b) {
            const int t0 = (int)((long long)b * n_keep / VAMP_EVID_BLOCKS), t1 = (int)((long long)(b + 1) * n_keep / VAMP_EVID_BLOCKS);
            zb[b] = 0.0;
            for (int j = 0; j + 1 < T; ++j) zb[b] += log_mean_exp(tr, T, W, j, t0, t1, betas[j + 1] - betas[j], red);
        }
    if (tid == 0) {
        lnZ[g] = z;
        double se = NAN;
        if (n_keep >= VAMP_EVID_BLOCKS) {
            double m = 0.0, v = 0.0;
            for (int b = 0; b < VAMP_EVID_BLOCKS; ++b) m += zb[b];
            m /= VAMP_EVID_BLOCKS;
            for (int b = 0; b < VAMP_EVID_BLOCKS; ++b) v += (zb[b] - m) * (zb[b] - m);
            se = sqrt(v / (VAMP_EVID_BLOCKS - 1)) / sqrt((double)VAMP_EVID_BLOCKS);
        }
        lnZ_se[g] = se;
        double ti = 0.0;
        for (int j = 0; j + 1 < T; ++j) ti += (betas[j + 1] - betas[j]) * 0.5 * (means[j] + means[j + 1]);
        lnZ_ti[g] = ti;
        for (int j = 0; j + 1 < T; ++j) {
            const int offered = n_swaps > j % 2 ? (n_swaps - j % 2 + 1) / 2 : 0;        // swaps n < n_swaps with n % 2 == j % 2
            swap_acc[g * (T - 1) + j] = offered ? (double)nswap[g * (T - 1) + j] / ((double)offered * (double)W) : NAN;
        }
    }
}

constexpr int kNarrowSlots = kWaves * (64 / vamp::kNarrowLanes) * slot_doubles(4 * vamp::kNarrowMaxK + 1, vamp::kNarrowMaxK, true);
constexpr int kWideSlots = kWaves * slot_doubles(kMaxD, VAMP_EVID_MAX_COMPONENTS, true);
constexpr size_t kStepsMaxLds =
    sizeof(double) * (size_t)(kHead + VAMP_EVID_MAX_WALKERS * (kMaxD + 2) + (kNarrowSlots > kWideSlots ? kNarrowSlots : kWideSlots));
constexpr size_t kDefaultLds = 64 * 1024;
// the checks of one region and its host-side record (pointers unset); `at` opens the message
int check_region(const std::string& at, const double* x, const double* flux, const double* noise, int P, int K, int mode, int sd,
                 const double* bounds, Reg& R) {
    if (!x || !flux) return fail(at + "NULL x or flux");
    if (P < 1) return fail(at + "n_pix must be positive");
    if (K < 1 || K > VAMP_EVID_MAX_COMPONENTS)
        return fail(at + "n_comp = " + std::to_string(K) + " is outside 1 .. " + std::to_string(VAMP_EVID_MAX_COMPONENTS));
    if (mode == 2) return fail(at + "mode 2 (NBZ3) is not supported: pass GAUSS3 (0) or VOIGT4 (1) parameters");
    if (mode != 0 && mode != 1) return fail(at + "mode must be 0 (GAUSS3) or 1 (VOIGT4)");
    if (sd != 0 && sd != 1) return fail(at + "sample_sd must be 0 or 1");
    if (!sd && !noise) return fail(at + "NULL noise");
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
    R.lanes = vamp::group_lanes(VAMP_EVID_NARROW, P, K);
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

// x | flux | weights of the regions into one device buffer; sets the three pointers of every record
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

size_t slots_bytes(const Reg& R) { return sizeof(double) * (size_t)kWaves * (64 / R.lanes) * slot_doubles(R.D, R.K, R.q == 4); }

}  // namespace

VAMP_EVID_API int vamp_evid_version(void) { return VAMP_EVID_ABI_VERSION; }

VAMP_EVID_API const char* vamp_evid_last_error(void) { return g_err.c_str(); }

VAMP_EVID_API int vamp_evid_default_betas(int n_temps, double* betas) {
    g_err.clear();
    if (n_temps < 2 || n_temps > VAMP_EVID_MAX_TEMPS)
        return fail("vamp_evid_default_betas: n_temps = " + std::to_string(n_temps) + " is outside 2 .. " + std::to_string(VAMP_EVID_MAX_TEMPS));
    if (!betas) return fail("vamp_evid_default_betas: NULL argument");
    for (int j = 0; j < n_temps; ++j) betas[j] = std::pow((double)j / (double)(n_temps - 1), 1.0 / 0.3);
    betas[0] = 0.0;
    betas[n_temps - 1] = 1.0;
    return 0;
}

VAMP_EVID_API int vamp_evid_lnlike(int device, const double* x, const double* flux, const double* noise, int n_pix, int n_comp, int mode,
                                   int sample_sd, const double* bounds, int n, const double* theta, double* lnlike, double* lnprior) {
    g_err.clear();
    const std::string fn = "vamp_evid_lnlike: ";
    if (n < 1) return fail(fn + "n must be positive");
    if (!theta || !lnlike || !lnprior) return fail(fn + "NULL argument");
    std::vector<Reg> regs(1);
    if (check_region(fn, x, flux, noise, n_pix, n_comp, mode, sample_sd, bounds, regs[0])) return -1;
    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = nullptr;
    DevBuf d_pix, d_regs, d_theta, d_out;
    std::vector<double> pix;
    if (upload_pixels(d_pix, regs, &x, &flux, &noise, st, pix)) return -1;
    const size_t D = regs[0].D;
    if (upload(d_regs, regs, st)) return -1;
    HIP_TRY(hipMalloc(&d_theta.p, (size_t)n * D * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(d_theta.p, theta, (size_t)n * D * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMalloc(&d_out.p, (size_t)n * 2 * sizeof(double)));
    const int blocks = (n + kEvalRows - 1) / kEvalRows;
    hipLaunchKernelGGL(k_evid_eval, dim3((unsigned)blocks), dim3(kBlock), slots_bytes(regs[0]), st, d_regs.as<Reg>(), blocks, kEvalRows, n,
                       d_theta.as<double>(), d_out.as<double>(), d_out.as<double>() + n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lnlike, d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lnprior, d_out.as<double>() + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

VAMP_EVID_API int vamp_evid_run(int device, void* hip_stream, int n_regions, const double* const* x, const double* const* flux,
                                const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                                const int32_t* sample_sd, const double* const* bounds, const int32_t* region_id, int n_temps,
                                const double* betas, int walkers, int n_steps, int burn, int swap_every, uint64_t seed, double a,
                                const double* const* start, double* lnZ, double* lnZ_se, double* lnZ_ti, double* mean_lnL, double* var_lnL,
                                double* move_accept, double* swap_accept, double* const* chain, double* const* chain_lnl, int chain_is_device,
                                double* lnl_trace, uint8_t* swap_trace) {
    g_err.clear();
    const std::string fn = "vamp_evid_run: ";
    const int G = n_regions, T = n_temps, W = walkers;
    if (G <= 0) return fail(fn + "n_regions must be positive");
    if (!x || !flux || !noise || !n_pix || !n_comp || !mode || !sample_sd || !region_id) return fail(fn + "NULL argument");
    if (T < 2 || T > VAMP_EVID_MAX_TEMPS) return fail(fn + "n_temps = " + std::to_string(T) + " is outside 2 .. " + std::to_string(VAMP_EVID_MAX_TEMPS));
    if (W < 4 || W > VAMP_EVID_MAX_WALKERS || (W & 1))
        return fail(fn + "walkers = " + std::to_string(W) + " must be even and in 4 .. " + std::to_string(VAMP_EVID_MAX_WALKERS));
    if (n_steps < 1 || burn < 0 || burn >= n_steps) return fail(fn + "n_steps must be positive and 0 <= burn < n_steps");
    if (swap_every < 1) return fail(fn + "swap_every must be positive");
    if (!(a > 1.0) || !std::isfinite(a)) return fail(fn + "the stretch scale a must exceed 1");
    std::vector<double> beta(T);
    if (betas) {
        for (int j = 0; j < T; ++j) beta[j] = betas[j];
        bool ok = beta[0] == 0.0 && beta[T - 1] == 1.0;
        for (int j = 1; j < T && ok; ++j) ok = beta[j] > beta[j - 1];
        if (!ok) return fail(fn + "betas must increase strictly from 0 to 1");
    } else if (vamp_evid_default_betas(T, beta.data())) return -1;
    const int n_keep = n_steps - burn, n_swaps = (n_steps - 1) / swap_every;
    std::vector<Reg> regs(G);
    long long theta_tot = 0, chain_tot = 0, cll_tot = 0;
    int D_max = 0;
    size_t lds_max = 0;
    for (int g = 0; g < G; ++g) {
        const std::string at = fn + "region " + std::to_string(g) + ": ";
        if (check_region(at, x[g], flux[g], noise[g], n_pix[g], n_comp[g], mode[g], sample_sd[g], bounds ? bounds[g] : nullptr, regs[g])) return -1;
        if (region_id[g] < 0 || ((long long)region_id[g] + 1) * T > 0x7fffffffLL) return fail(at + "region_id is negative or too large for the draw keys");
        Reg& R = regs[g];
        R.rid = (unsigned)region_id[g];
        R.theta_off = theta_tot;
        R.out_off = (long long)g * T * W;
        theta_tot += (long long)T * W * R.D;
        D_max = R.D > D_max ? R.D : D_max;
        if (start && start[g])
            for (long long i = 0; i < (long long)W * R.D; ++i)
                if (!std::isfinite(start[g][i])) return fail(at + "the start is not finite");
        const size_t lds = sizeof(double) * ((size_t)kHead + (size_t)W * (R.D + 2)) + slots_bytes(R);
        lds_max = lds > lds_max ? lds : lds_max;
        if (chain && chain[g]) chain_tot += (long long)n_keep * W * R.D;
        if (chain_lnl && chain_lnl[g]) cll_tot += (long long)n_keep * W;
    }
    const long long trace_len = (long long)G * n_keep * T * W;
    const long long swap_len = (long long)G * n_swaps * (T - 1) * W;
    if ((long long)G * T > 0x7fffffffLL / kBlock || trace_len > (1LL << 40)) return fail(fn + "too much work for one call");

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    // k_evid_steps may ask for more dynamic LDS than a launch gets by default
    if (lds_max > kDefaultLds && raise_lds_limit(fn, device, {{reinterpret_cast<const void*>(&k_evid_steps), kStepsMaxLds}})) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    DevBuf d_pix, d_regs, d_beta, d_start, d_startp, d_X, d_ll, d_trace, d_cnt, d_out, d_chain, d_swaptr;
    std::vector<double> pix;
    if (upload_pixels(d_pix, regs, x, flux, noise, st, pix)) return -1;
    // the beta = 1 chains: the caller's device memory, or one staging buffer copied back at the end
    if (!chain_is_device && chain_tot + cll_tot > 0) HIP_TRY(hipMalloc(&d_chain.p, (size_t)(chain_tot + cll_tot) * sizeof(double)));
    {
        long long o = 0;
        for (int g = 0; g < G; ++g) {
            Reg& R = regs[g];
            if (chain && chain[g]) {
                R.chain = chain_is_device ? chain[g] : d_chain.as<double>() + o;
                o += chain_is_device ? 0 : (long long)n_keep * W * R.D;
            }
            if (chain_lnl && chain_lnl[g]) {
                R.chain_ll = chain_is_device ? chain_lnl[g] : d_chain.as<double>() + o;
                o += chain_is_device ? 0 : (long long)n_keep * W;
            }
        }
    }
    if (upload(d_regs, regs, st) || upload(d_beta, beta, st)) return -1;
    // the start blocks, one after the other, and a device table of their addresses (NULL: prior draws)
    std::vector<double> start_h;
    std::vector<const double*> start_p(G, nullptr);
    {
        std::vector<long long> off(G, -1);
        for (int g = 0; g < G; ++g)
            if (start && start[g]) {
                off[g] = (long long)start_h.size();
                start_h.insert(start_h.end(), start[g], start[g] + (long long)W * regs[g].D);
            }
        if (upload(d_start, start_h, st)) return -1;
        for (int g = 0; g < G; ++g)
            if (off[g] >= 0) start_p[g] = d_start.as<double>() + off[g];
        if (upload(d_startp, start_p, st)) return -1;
    }
    const long long n_walk = (long long)G * T * W;
    HIP_TRY(hipMalloc(&d_X.p, (size_t)theta_tot * sizeof(double)));
    HIP_TRY(hipMalloc(&d_ll.p, (size_t)n_walk * 2 * sizeof(double)));
    HIP_TRY(hipMalloc(&d_trace.p, (size_t)trace_len * sizeof(double)));
    const size_t n_cnt = (size_t)G * T + (size_t)G * (T - 1);
    HIP_TRY(hipMalloc(&d_cnt.p, n_cnt * sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(d_cnt.p, 0, n_cnt * sizeof(unsigned), st));
    if (swap_trace && swap_len > 0) {
        HIP_TRY(hipMalloc(&d_swaptr.p, (size_t)swap_len));
        HIP_TRY(hipMemsetAsync(d_swaptr.p, 0, (size_t)swap_len, st));
    }
    double* dX = d_X.as<double>();
    double* dll = d_ll.as<double>();
    double* dlp = dll + n_walk;
    unsigned* nacc = d_cnt.as<unsigned>();
    unsigned* nswap = nacc + (size_t)G * T;
    const Reg* dregs = d_regs.as<Reg>();

    hipLaunchKernelGGL(k_evid_init, dim3((unsigned)((n_walk + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dregs,
                       d_startp.as<const double*>(), T, W, (unsigned long long)seed, dX, n_walk);
    HIP_TRY(hipGetLastError());
    size_t eval_lds = 0;
    for (const Reg& R : regs) eval_lds = slots_bytes(R) > eval_lds ? slots_bytes(R) : eval_lds;
    hipLaunchKernelGGL(k_evid_eval, dim3((unsigned)(G * T)), dim3(kBlock), eval_lds, st, dregs, T, W, T * W, dX, dll, dlp);
    HIP_TRY(hipGetLastError());
    {   // every start point inside the prior, with a finite ln L
        std::vector<double> h((size_t)n_walk * 2);
        HIP_TRY(hipMemcpyAsync(h.data(), dll, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (long long i = 0; i < n_walk; ++i)
            if (!(h[n_walk + i] > -INFINITY) || !std::isfinite(h[i]))
                return fail(fn + "region " + std::to_string(i / ((long long)T * W)) + ": start walker " + std::to_string(i % W) + " of rung " +
                            std::to_string((i / W) % T) + (h[n_walk + i] > -INFINITY ? " has no finite ln L" : " is outside the prior"));
    }
    int swap_n = 0;
    for (int s0 = 0; s0 < n_steps; s0 += swap_every) {
        const int ns = n_steps - s0 < swap_every ? n_steps - s0 : swap_every;
        hipLaunchKernelGGL(k_evid_steps, dim3((unsigned)(G * T)), dim3(kBlock), lds_max, st, dregs, d_beta.as<double>(), T, W,
                           (unsigned long long)seed, a, s0, ns, burn, n_keep, dX, dll, dlp, d_trace.as<double>(), nacc);
        HIP_TRY(hipGetLastError());
        if (swap_n < n_swaps) {
            const int n_pairs = (T - 1 - (swap_n & 1) + 1) / 2;        // pairs (j, j + 1), j = parity, parity + 2, ... <= T - 2
            const long long total = (long long)G * n_pairs * W;
            if (total > 0) {
                hipLaunchKernelGGL(k_evid_swap, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dregs, d_beta.as<double>(),
                                   T, W, (unsigned long long)seed, (unsigned)swap_n, n_pairs, dX, dll, dlp, nswap, d_swaptr.as<uint8_t>(),
                                   n_swaps, total);
                HIP_TRY(hipGetLastError());
            }
            ++swap_n;
        }
    }
    // lnZ | se | ti | mean | var | move | swap
    const long long o_z = 0, o_se = G, o_ti = 2LL * G, o_m = 3LL * G, o_v = o_m + (long long)G * T, o_ma = o_v + (long long)G * T,
                    o_sa = o_ma + (long long)G * T, o_end = o_sa + (long long)G * (T - 1);
    HIP_TRY(hipMalloc(&d_out.p, (size_t)o_end * sizeof(double)));
    double* dout = d_out.as<double>();
    hipLaunchKernelGGL(k_evid_reduce, dim3((unsigned)G), dim3(kBlock), 0, st, d_beta.as<double>(), T, W, n_keep, n_steps, n_swaps,
                       d_trace.as<double>(), nacc, nswap, dout + o_z, dout + o_se, dout + o_ti, dout + o_m, dout + o_v, dout + o_ma, dout + o_sa);
    HIP_TRY(hipGetLastError());

    const long long sz = sizeof(double);
    if (fetch(lnZ, dout + o_z, G * sz, st) || fetch(lnZ_se, dout + o_se, G * sz, st) || fetch(lnZ_ti, dout + o_ti, G * sz, st) ||
        fetch(mean_lnL, dout + o_m, (long long)G * T * sz, st) || fetch(var_lnL, dout + o_v, (long long)G * T * sz, st) ||
        fetch(move_accept, dout + o_ma, (long long)G * T * sz, st) || fetch(swap_accept, dout + o_sa, (long long)G * (T - 1) * sz, st) ||
        fetch(lnl_trace, d_trace.p, trace_len * sz, st) || fetch(swap_trace, d_swaptr.p, swap_len, st))
        return -1;
    if (!chain_is_device)
        for (int g = 0; g < G; ++g) {
            const Reg& R = regs[g];
            if (R.chain && fetch(chain[g], R.chain, (long long)n_keep * W * R.D * sz, st)) return -1;
            if (R.chain_ll && fetch(chain_lnl[g], R.chain_ll, (long long)n_keep * W * sz, st)) return -1;
        }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
