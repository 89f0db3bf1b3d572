// hmc.hip -- Hamiltonian Monte Carlo chains per region: C chains per group, L leapfrog steps per move in the metric of
// a given factor, the exact log-posterior and its analytic gradient (include/vamp_hmc.h, libvamp_hmc.so).  Definitions:
// the header, and DESIGN.md section 17.
//
// A call is one launch of k_hmc: the whole step loop is resident.  One 64-lane wavefront owns one chain; a workgroup holds
// up to four chains of one group (fewer when the call's largest D would not leave them room in LDS) and stages the
// packed lower triangle of the factor once.  Per wavefront, in LDS and ordered by lds_fence(): the state theta, its
// gradient g, the trajectory's theta', g' and momentum p, the line records and near-axis tables of the point being
// evaluated, and the tile of d tau / d theta of 64 pixels.  One evaluation (eval_point) is
//   1. the records and the prior of the lines (laplace.hip's rule), a lane per line; outside the prior it ends here
//   2. the near-axis tables; then the pixels in tiles of 64, one per lane: every line's voigt_grad value gives its share
//      of tau and its four derivative terms, which go to the lane's column of the tile; f = exp(-tau), the residual,
//      the lane's share of chi^2 and the pixel's weight -f r / sigma^2
//   3. lane d folds row d of the tile with the weights in pixel order (VAMP_HMC_TREE = 1: a butterfly of fixed order per
//      row instead; tools/bench_hmc.py compares the two), tile after tile in registers
//   4. chi^2 by a butterfly; ln p; the prior's terms and the free sd's entry of the gradient.
// Every loop has a trip count fixed before the launch but the early exit at a wall.  Everything is fp64; results leave
// the kernel by ordinary vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_hmc.h"
#include "draws.hpp"
#include "lane_group.hpp"
#include "side_call.hpp"
#include "voigt_grad.hpp"
#include "voigt_math.hpp"

#define VAMP_HMC_API extern "C" __attribute__((visibility("default")))

// 0: lane d folds the tile's row d in pixel order; 1: a butterfly over the lanes per row (tools/bench_hmc.py)
#ifndef VAMP_HMC_TREE
#define VAMP_HMC_TREE 0
#endif

namespace {

using namespace vamp::side;
using vamp::lds_fence;

constexpr int kMaxWaves = 4;               // chains of a workgroup
constexpr int kTile = 64;                  // pixels of a tile: one per lane
constexpr int kTileStride = kTile + 1;     // doubles between two rows of the tile: lane d on row d hits its own bank
constexpr int kRec = 7;                    // doubles of a line record: centre, scale, damping, amplitude, pole, h y, ln prior
constexpr int kMaxD = VAMP_HMC_MAX_DIM;
constexpr int kMaxK = VAMP_HMC_MAX_COMPONENTS;
constexpr double SQRT_LN2 = 0.83255461115769775635;
constexpr unsigned STREAM_MOMENTUM = 6, STREAM_HMC_ACCEPT = 7;      // beside 0 - 5 of draws.hpp, evidence.hip and laplace.hip
constexpr size_t kLdsBudget = 160 * 1024 - 1024;                    // of a CU's 160 KiB
static_assert(kMaxD == 4 * kMaxK + 1, "D = q K + sd");

struct Grp {                       // one group
    const double* x;               // device: abscissa, flux, 1 / noise (1 with the free sd)
    const double* f;
    const double* wt;
    const double* C;               // device: the packed lower triangle, C_de at d (d + 1) / 2 + e
    const double* start;           // device [C][D]
    const double* mom_in;          // device [n_steps][C][D], or NULL
    double *chain, *last, *lnp;    // device, or NULL
    double *mom, *prop, *prop_mom, *dH;
    int32_t* acc;
    long long o_chain;             // where the group's first chain stands in the per-chain outputs
    double c_lo, c_hi, w_max, lp_c, lp_w, norm_const;
    double eps, jitter;
    int P, K, q, D, sd, nC;        // nC: chains
    int skip;                      // 1: no factor (status 1)
    unsigned rid, cid0;
};

struct PerChain {                  // the per-chain outputs of the call
    int32_t *n_accept, *n_wall, *status;
    double *dH_mean, *dH_max;
};

struct Steps {
    int n_leap, n_steps, n_burn, thin, n_keep;
    unsigned step0, k0, k1;
};

// doubles of a wavefront's LDS: theta, g, theta', g', p; the records; the tables; the tile; the weights
__host__ __device__ constexpr int slot_doubles(int D, int K, bool voigt) {
    return 5 * D + K * kRec + (voigt ? K * vamp::DTAB_N : 0) + (voigt ? 4 : 3) * K * kTileStride + kTile;
}
__host__ __device__ constexpr int head_doubles(int D) { return D * (D + 1) / 2; }
static_assert(sizeof(double) * (head_doubles(kMaxD) + slot_doubles(kMaxD, kMaxK, true)) <= kLdsBudget, "one chain of the largest D fits");

__device__ __forceinline__ double xexp_logp(double v) {        // log(v exp(-v)), literally; -inf below 0
    if (!(v >= 0.0) || !isfinite(v)) return -INFINITY;
    return log(v * exp(-v));
}
__device__ __forceinline__ double uniform_logp(double v, double lo, double hi, double lp) { return (v >= lo && v <= hi) ? lp : -INFINITY; }

struct Slot {                      // a wavefront's LDS
    double *th, *g, *thn, *gn, *p, *rec, *dtab, *tile, *sw;
};

// ln p of the parameters q[D] (LDS) and its gradient into gout[D] (LDS), by the 64 lanes of one wavefront; all lanes
// return the same values.  false: the point is rejected (outside the prior, bad, or ln p not finite); gout is then not
// to be read.
__device__ __forceinline__ bool eval_point(const Grp& R, const Slot& S, const double* q, double* gout, int lane, double& lnp_out) {
    const bool voigt = R.q == 4;
    const int K = R.K, nq = R.q, Dl = nq * K;
    for (int k = lane; k < K; k += 64) {
        const double* th = q + nq * k;
        const double a = th[0], c = th[1];
        double* r = S.rec + k * kRec;
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
    for (int k = 0; k < K; ++k) lp += S.rec[k * kRec + 6];
    const double sd = R.sd ? q[R.D - 1] : 1.0;
    if (R.sd) lp += uniform_logp(sd, 0.0, 1.0, 0.0);
    if (!(lp > -INFINITY)) {                       // (uniform; false for NaN too)
        lds_fence();
        return false;
    }
    if (voigt) vamp::fill_dtab<kRec>(S.dtab, S.rec, K, lane, 64);
    lds_fence();

    double chi = 0.0, gacc = 0.0;
    for (int p0 = 0; p0 < R.P; p0 += kTile) {
        const int np = min(kTile, R.P - p0);
        double w = 0.0;
        if (lane < np) {
            const double xi = R.x[p0 + lane];
            double tau = 0.0;
            for (int k = 0; k < K; ++k) {
                const double* r = S.rec + k * kRec;
                const double* th = q + nq * k;
                double* a = S.tile + (nq * k) * kTileStride + lane;
                const double u = (xi - r[0]) * r[1];
                if (voigt) {
                    const vamp::VoigtGrad vg = vamp::voigt_grad(u, r[2], S.dtab + k * vamp::DTAB_N, r[4], r[5]);
                    tau += r[3] * vg.Ks;
                    a[0] = r[2] * vg.Ks;
                    a[kTileStride] = -(r[3] * vamp::SQRT_PI) * r[1] * vg.Ku;
                    a[2 * kTileStride] = (th[0] * vamp::SQRT_PI) * (0.5 * r[1]) * vg.TL;
                    a[3 * kTileStride] = -((r[3] * vamp::SQRT_PI) / th[3]) * vg.TG;
                } else {
                    const double e = exp(-0.5 * (u * u));
                    const double ae = th[0] * e;
                    tau += ae;
                    a[0] = e;
                    a[kTileStride] = ae * u * r[1];
                    a[2 * kTileStride] = ae * (u * u) * r[1];
                }
            }
            const double f = exp(-tau);
            const double wt = R.wt[p0 + lane];
            const double rs = (R.f[p0 + lane] - f) * wt;
            chi = fma(rs, rs, chi);
            w = -f * (rs * wt);
        }
        S.sw[lane] = w;
        lds_fence();
#if VAMP_HMC_TREE
        for (int d = 0; d < Dl; ++d) {
            double v = lane < np ? S.tile[d * kTileStride + lane] * w : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == d) gacc += v;
        }
#else
        if (lane < Dl) {
            const double* row = S.tile + lane * kTileStride;
            for (int p = 0; p < np; ++p) gacc = fma(row[p], S.sw[p], gacc);
        }
#endif
        lds_fence();                               // the tile is free for the next pixels
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) chi += __shfl_xor(chi, o, 64);

    double ll;
    const double t = 1.0 / (sd * sd);
    if (R.sd) ll = (double)R.P * 0.5 * log(t / (2.0 * vamp::PI)) - 0.5 * t * chi;
    else ll = -0.5 * chi + R.norm_const;
    const double lnp = lp + ll;
    if (lane < Dl) {
        double gd = R.sd ? gacc * t : gacc;
        if (lane % nq == 0) gd += 1.0 / q[lane] - 1.0;
        gout[lane] = gd;
    }
    if (R.sd && lane == 0) gout[Dl] = chi / (sd * sd * sd) - (double)R.P / sd;
    lds_fence();
    lnp_out = lnp;
    return isfinite(ll) && isfinite(lnp);
}

// p_e <- fma(h, (C^T g)_e, p_e)
__device__ __forceinline__ void kick(const double* Cs, const double* g, double* p, int D, double h, int lane) {
    for (int e = lane; e < D; e += 64) {
        double v = 0.0;
        for (int d = e; d < D; ++d) v = fma(Cs[d * (d + 1) / 2 + e], g[d], v);
        p[e] = fma(h, v, p[e]);
    }
    lds_fence();
}

// theta_d <- fma(eps, (C p)_d, theta_d)
__device__ __forceinline__ void drift(const double* Cs, const double* p, double* th, int D, double eps, int lane) {
    for (int d = lane; d < D; d += 64) {
        const double* Cd = Cs + d * (d + 1) / 2;
        double w = 0.0;
        for (int e = 0; e <= d; ++e) w = fma(Cd[e], p[e], w);
        th[d] = fma(eps, w, th[d]);
    }
    lds_fence();
}

__device__ __forceinline__ double kinetic(const double* p, int D) {
    double k = 0.0;
    for (int d = 0; d < D; ++d) k = fma(p[d], p[d], k);
    return k;
}

// Dynamic LDS: the packed C, then one slot per wavefront.  task: (group, first chain of the workgroup)
__global__ __launch_bounds__(64 * kMaxWaves) void k_hmc(const Grp* __restrict__ grps, const int2* __restrict__ tasks, Steps T, PerChain out) {
    extern __shared__ double lds[];
    const int2 task = tasks[blockIdx.x];
    const Grp R = grps[task.x];
    const int D = R.D, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool voigt = R.q == 4;
    const int nC = head_doubles(D);
    if (!R.skip)
        for (int i = tid; i < nC; i += blockDim.x) lds[i] = R.C[i];
    __syncthreads();                               // the only barrier: a wavefront is on its own from here
    const int ci = task.y + wave;                  // the chain's index in its group
    if (ci >= R.nC) return;

    const long long oc = R.o_chain + ci;
    const long long CD = (long long)R.nC * D;
    Slot S;
    S.th = lds + nC + (size_t)wave * slot_doubles(D, R.K, voigt);
    S.g = S.th + D; S.thn = S.g + D; S.gn = S.thn + D; S.p = S.gn + D;
    S.rec = S.p + D;
    S.dtab = S.rec + R.K * kRec;
    S.tile = S.dtab + (voigt ? R.K * vamp::DTAB_N : 0);
    S.sw = S.tile + R.q * R.K * kTileStride;
    const double* Cs = lds;

    double lnp = NAN;
    bool ok = !R.skip;
    if (ok) {
        for (int d = lane; d < D; d += 64) S.th[d] = R.start[(long long)ci * D + d];
        lds_fence();
        ok = eval_point(R, S, S.th, S.g, lane, lnp);
    }
    if (!ok) {                                     // (uniform) status 1 of the group or 2 of the chain: NaN everywhere
        for (int i = 0; i < T.n_keep; ++i) {
            if (R.chain) for (int d = lane; d < D; d += 64) R.chain[i * CD + (long long)ci * D + d] = NAN;
            if (R.lnp && lane == 0) R.lnp[(long long)i * R.nC + ci] = NAN;
        }
        for (int t = 0; t < T.n_steps; ++t) {
            for (int d = lane; d < D; d += 64) {
                const long long at = t * CD + (long long)ci * D + d;
                if (R.mom) R.mom[at] = NAN;
                if (R.prop) R.prop[at] = NAN;
                if (R.prop_mom) R.prop_mom[at] = NAN;
            }
            if (lane == 0) {
                if (R.dH) R.dH[(long long)t * R.nC + ci] = NAN;
                if (R.acc) R.acc[(long long)t * R.nC + ci] = 0;
            }
        }
        if (R.last) for (int d = lane; d < D; d += 64) R.last[(long long)ci * D + d] = NAN;
        if (lane == 0) {
            out.n_accept[oc] = 0; out.n_wall[oc] = 0; out.status[oc] = R.skip ? 1 : 2;
            out.dH_mean[oc] = NAN; out.dH_max[oc] = NAN;
        }
        return;
    }

    const unsigned cid = R.cid0 + (unsigned)ci;
    int n_acc = 0, n_wall = 0, kept = 0;
    double dh_sum = 0.0, dh_max = 0.0;
    for (int t = 0; t < T.n_steps; ++t) {
        const unsigned tt = T.step0 + (unsigned)t;
        const long long row = t * CD + (long long)ci * D;
        // the momentum
        if (R.mom_in) {
            for (int d = lane; d < D; d += 64) S.p[d] = R.mom_in[row + d];
        } else {
            for (int j = lane; 2 * j < D; j += 64) {
                const vamp::U4 r = vamp::philox4x32_10({tt, cid * 64u + (unsigned)j, STREAM_MOMENTUM, R.rid}, T.k0, T.k1);
                const double u1 = 1.0 - vamp::u53(r.c0, r.c1), u2 = vamp::u53(r.c2, r.c3);
                const double rho = sqrt(-2.0 * log(u1));
                double sn, cs;
                sincos((2.0 * vamp::PI) * u2, &sn, &cs);
                S.p[2 * j] = rho * cs;
                if (2 * j + 1 < D) S.p[2 * j + 1] = rho * sn;
            }
        }
        for (int d = lane; d < D; d += 64) { S.thn[d] = S.th[d]; S.gn[d] = S.g[d]; }
        lds_fence();
        if (R.mom) for (int d = lane; d < D; d += 64) R.mom[row + d] = S.p[d];
        const vamp::U4 ra = vamp::philox4x32_10({tt, cid * 64u + 63u, STREAM_HMC_ACCEPT, R.rid}, T.k0, T.k1);
        const double u = 1.0 - vamp::u53(ra.c0, ra.c1), u2 = vamp::u53(ra.c2, ra.c3);
        const double eps = R.eps * (1.0 + R.jitter * (2.0 * u2 - 1.0));
        const double H0 = lnp - 0.5 * kinetic(S.p, D);
        kick(Cs, S.gn, S.p, D, 0.5 * eps, lane);
        double lnpn = NAN;
        bool wall = false;
        for (int l = 0; l < T.n_leap; ++l) {
            drift(Cs, S.p, S.thn, D, eps, lane);
            if (!eval_point(R, S, S.thn, S.gn, lane, lnpn)) { wall = true; break; }      // (uniform) the one early exit
            kick(Cs, S.gn, S.p, D, l + 1 < T.n_leap ? eps : 0.5 * eps, lane);
        }
        const double dH = wall ? NAN : (lnpn - 0.5 * kinetic(S.p, D)) - H0;
        const bool accept = !wall && log(u) < dH;
        for (int d = lane; d < D; d += 64) {
            if (R.prop) R.prop[row + d] = S.thn[d];
            if (R.prop_mom) R.prop_mom[row + d] = S.p[d];
        }
        if (lane == 0) {
            if (R.dH) R.dH[(long long)t * R.nC + ci] = dH;
            if (R.acc) R.acc[(long long)t * R.nC + ci] = wall ? 2 : (accept ? 1 : 0);
        }
        if (wall) {
            ++n_wall;
        } else {
            dh_sum += fabs(dH);
            dh_max = fmax(dh_max, fabs(dH));
        }
        lds_fence();
        if (accept) {
            ++n_acc;
            lnp = lnpn;
            for (int d = lane; d < D; d += 64) { S.th[d] = S.thn[d]; S.g[d] = S.gn[d]; }
            lds_fence();
        }
        if (t >= T.n_burn && (t - T.n_burn) % T.thin == 0) {
            if (R.chain) for (int d = lane; d < D; d += 64) R.chain[kept * CD + (long long)ci * D + d] = S.th[d];
            if (R.lnp && lane == 0) R.lnp[(long long)kept * R.nC + ci] = lnp;
            ++kept;
        }
    }
    if (R.last) for (int d = lane; d < D; d += 64) R.last[(long long)ci * D + d] = S.th[d];
    if (lane == 0) {
        const int n_free = T.n_steps - n_wall;
        out.n_accept[oc] = n_acc; out.n_wall[oc] = n_wall; out.status[oc] = 0;
        out.dH_mean[oc] = n_free > 0 ? dh_sum / (double)n_free : NAN;
        out.dH_max[oc] = n_free > 0 ? dh_max : NAN;
    }
}

// the checks of one group's data and its host-side record (pointers unset); `at` opens the message
int check_region(const std::string& at, const double* x, const double* flux, const double* noise, int P, int K, int mode, int sd,
                 const double* bounds, Grp& R) {
    if (!x || !flux) return fail(at + "NULL x or flux");
    if (P < 1) return fail(at + "n_pix must be positive");
    if (K < 1 || K > kMaxK) return fail(at + "n_comp = " + std::to_string(K) + " is outside 1 .. " + std::to_string(kMaxK));
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
    R = Grp{};
    R.P = P; R.K = K; R.q = mode == 1 ? 4 : 3; R.sd = sd; R.D = R.q * K + sd;
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

// the factor of one group into `packed` (the lower triangle row by row); false: no factor (status 1)
bool pack_factor(const double* chol, int D, std::vector<double>& packed) {
    const size_t at = packed.size();
    packed.resize(at + (size_t)head_doubles(D), 0.0);
    for (int d = 0; d < D; ++d) {
        for (int e = 0; e <= d; ++e)
            if (!std::isfinite(chol[(size_t)d * D + e])) return false;
        if (!(chol[(size_t)d * D + d] > 0.0)) return false;
    }
    double* dst = packed.data() + at;
    for (int d = 0; d < D; ++d)
        for (int e = 0; e <= d; ++e) *dst++ = chol[(size_t)d * D + e];
    return true;
}

size_t lds_bytes(int D, int K, bool voigt, int waves) { return sizeof(double) * ((size_t)head_doubles(D) + (size_t)waves * slot_doubles(D, K, voigt)); }

}  // namespace

VAMP_HMC_API int vamp_hmc_version(void) { return VAMP_HMC_ABI_VERSION; }

VAMP_HMC_API const char* vamp_hmc_last_error(void) { return g_err.c_str(); }

VAMP_HMC_API int vamp_hmc_chains(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                                 const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                                 const int32_t* sample_sd, const double* const* bounds, const int32_t* region_id, const int32_t* n_chains,
                                 const int32_t* chain_id0, const double* const* start, int start_is_device, const double* const* chol,
                                 const double* eps, const double* jitter, int n_leap, int n_steps, int n_burn, int thin, int64_t step0,
                                 uint64_t seed, const double* const* mom_in, double* const* chain, double* const* last, int out_is_device,
                                 double* const* lnp, int32_t* n_accept, int32_t* n_wall, double* dH_mean, double* dH_max,
                                 int32_t* chain_status, int32_t* status, double* const* mom, double* const* prop, double* const* prop_mom,
                                 double* const* dH, int32_t* const* acc) {
    g_err.clear();
    const std::string fn = "vamp_hmc_chains: ";
    const int G = n_groups;
    if (G <= 0) return fail(fn + "n_groups must be positive");
    if (!x || !flux || !noise || !n_pix || !n_comp || !mode || !sample_sd || !region_id || !n_chains || !chain_id0 || !start || !chol || !eps ||
        !jitter)
        return fail(fn + "NULL argument");
    if (n_leap < 1 || n_leap > VAMP_HMC_MAX_LEAP)
        return fail(fn + "n_leap = " + std::to_string(n_leap) + " is outside 1 .. " + std::to_string(VAMP_HMC_MAX_LEAP));
    if (n_steps < 1) return fail(fn + "n_steps must be positive");
    if (n_burn < 0 || n_burn >= n_steps) return fail(fn + "n_burn = " + std::to_string(n_burn) + " is outside 0 .. n_steps - 1");
    if (thin < 1) return fail(fn + "thin must be at least 1");
    if (step0 < 0 || step0 + (int64_t)n_steps > (1LL << 31)) return fail(fn + "step0 + n_steps is outside 0 .. 2^31");
    if (start_is_device != 0 && start_is_device != 1) return fail(fn + "start_is_device must be 0 or 1");
    if (out_is_device != 0 && out_is_device != 1) return fail(fn + "out_is_device must be 0 or 1");
    const int n_keep = (n_steps - n_burn + thin - 1) / thin;
    const bool traces = mom_in || mom || prop || prop_mom;

    std::vector<Grp> grps(G);
    std::vector<double> packed;
    std::vector<long long> head_off(G);
    std::vector<int32_t> st_host(G);
    long long tot_chains = 0, tot_keep = 0, tot_steps = 0;
    for (int g = 0; g < G; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        Grp& R = grps[g];
        if (check_region(at, x[g], flux[g], noise[g], n_pix[g], n_comp[g], mode[g], sample_sd[g], bounds ? bounds[g] : nullptr, R)) return -1;
        if (region_id[g] < 0) return fail(at + "region_id is negative");
        if (n_chains[g] < 1) return fail(at + "n_chains must be at least 1");
        if (chain_id0[g] < 0 || (long long)chain_id0[g] + n_chains[g] > VAMP_HMC_MAX_CHAIN_ID)
            return fail(at + "chain identities must lie in 0 .. 2^26 - 1");
        if (!start[g] || !chol[g]) return fail(at + "NULL start or chol");
        R.rid = (unsigned)region_id[g];
        R.cid0 = (unsigned)chain_id0[g];
        R.nC = n_chains[g];
        R.eps = eps[g]; R.jitter = jitter[g];
        head_off[g] = (long long)packed.size();
        const bool factor = pack_factor(chol[g], R.D, packed);
        R.skip = (factor && std::isfinite(R.eps) && R.eps > 0.0 && R.jitter >= 0.0 && R.jitter < 1.0) ? 0 : 1;
        st_host[g] = R.skip;
        R.o_chain = tot_chains;
        tot_chains += R.nC;
        tot_keep += (long long)n_keep * R.nC * R.D;
        tot_steps += (long long)n_steps * R.nC * R.D;
        if (tot_keep > VAMP_HMC_MAX_CHAIN_DOUBLES)
            return fail(fn + "more than " + std::to_string(VAMP_HMC_MAX_CHAIN_DOUBLES) + " doubles of kept states (sum of n_keep C D): split the call");
        if (traces && tot_steps > VAMP_HMC_MAX_CHAIN_DOUBLES)
            return fail(fn + "more than " + std::to_string(VAMP_HMC_MAX_CHAIN_DOUBLES) + " doubles in a trace (sum of n_steps C D): split the call");
        if (tot_chains > (1LL << 30)) return fail(fn + "too many chains");
    }
    // chains of a workgroup: as many of the four as the call's largest group leaves room for
    int waves = kMaxWaves;
    size_t lds = 0;
    for (;; --waves) {
        lds = 0;
        for (const Grp& R : grps) lds = std::max(lds, lds_bytes(R.D, R.K, R.q == 4, waves));
        if (lds <= kLdsBudget || waves == 1) break;
    }

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (raise_lds_limit(fn, device, {{reinterpret_cast<const void*>(&k_hmc), kLdsBudget}})) return -1;

    // the pixels: x | flux | weights
    long long tot_pix = 0;
    for (const Grp& R : grps) tot_pix += R.P;
    std::vector<double> pix((size_t)tot_pix * 3);
    {
        long long o = 0;
        for (int g = 0; g < G; ++g) {
            const Grp& R = grps[g];
            for (int p = 0; p < R.P; ++p) {
                pix[o + p] = x[g][p];
                pix[tot_pix + o + p] = flux[g][p];
                pix[2 * tot_pix + o + p] = R.sd ? 1.0 : 1.0 / noise[g][p];
            }
            o += R.P;
        }
    }
    DevBuf d_pix, d_packed, d_grps, d_tasks, d_start, d_momin, d_dbl, d_int;
    if (upload(d_pix, pix, st) || upload(d_packed, packed, st)) return -1;

    // device views of the starts and of the given momenta
    std::vector<const double*> dstart(start, start + G), dmomin(G, nullptr);
    if (!start_is_device) {
        std::vector<long long> len(G);
        for (int g = 0; g < G; ++g) len[g] = (long long)grps[g].nC * grps[g].D;
        if (stage_chains(len, start, st, d_start, dstart)) return -1;
    }
    if (mom_in) {
        std::vector<long long> len(G);
        for (int g = 0; g < G; ++g) len[g] = mom_in[g] ? (long long)n_steps * grps[g].nC * grps[g].D : 0;
        if (stage_chains(len, mom_in, st, d_momin, dmomin)) return -1;
    }

    // one buffer of doubles for every output the library holds itself, one of int32
    auto want = [](double* const* list, int g) { return list && list[g]; };
    std::vector<long long> o_chain(G, -1), o_last(G, -1), o_lnp(G, -1), o_mom(G, -1), o_prop(G, -1), o_pm(G, -1), o_dH(G, -1), o_acc(G, -1);
    long long nd = 2 * tot_chains, ni = 3 * tot_chains;      // dH_mean | dH_max; n_accept | n_wall | chain_status
    for (int g = 0; g < G; ++g) {
        const Grp& R = grps[g];
        const long long keep = (long long)n_keep * R.nC, steps = (long long)n_steps * R.nC;
        if (want(chain, g) && !out_is_device) { o_chain[g] = nd; nd += keep * R.D; }
        if (want(last, g) && !out_is_device) { o_last[g] = nd; nd += (long long)R.nC * R.D; }
        if (want(lnp, g)) { o_lnp[g] = nd; nd += keep; }
        if (want(mom, g)) { o_mom[g] = nd; nd += steps * R.D; }
        if (want(prop, g)) { o_prop[g] = nd; nd += steps * R.D; }
        if (want(prop_mom, g)) { o_pm[g] = nd; nd += steps * R.D; }
        if (want(dH, g)) { o_dH[g] = nd; nd += steps; }
        if (acc && acc[g]) { o_acc[g] = ni; ni += steps; }
    }
    HIP_TRY(hipMalloc(&d_dbl.p, (size_t)nd * sizeof(double)));
    HIP_TRY(hipMalloc(&d_int.p, (size_t)ni * sizeof(int32_t)));
    double* dd = d_dbl.as<double>();
    int32_t* di = d_int.as<int32_t>();

    std::vector<int2> tasks;
    {
        long long o = 0;
        for (int g = 0; g < G; ++g) {
            Grp& R = grps[g];
            R.x = d_pix.as<double>() + o; R.f = R.x + tot_pix; R.wt = R.x + 2 * tot_pix;
            o += R.P;
            R.C = d_packed.as<double>() + head_off[g];
            R.start = dstart[g];
            R.mom_in = dmomin[g];
            R.chain = want(chain, g) ? (out_is_device ? chain[g] : dd + o_chain[g]) : nullptr;
            R.last = want(last, g) ? (out_is_device ? last[g] : dd + o_last[g]) : nullptr;
            R.lnp = o_lnp[g] >= 0 ? dd + o_lnp[g] : nullptr;
            R.mom = o_mom[g] >= 0 ? dd + o_mom[g] : nullptr;
            R.prop = o_prop[g] >= 0 ? dd + o_prop[g] : nullptr;
            R.prop_mom = o_pm[g] >= 0 ? dd + o_pm[g] : nullptr;
            R.dH = o_dH[g] >= 0 ? dd + o_dH[g] : nullptr;
            R.acc = o_acc[g] >= 0 ? di + o_acc[g] : nullptr;
            for (int c = 0; c < R.nC; c += waves) tasks.push_back(make_int2(g, c));
        }
    }
    if (tasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");
    if (upload(d_grps, grps, st) || upload(d_tasks, tasks, st)) return -1;

    Steps T;
    T.n_leap = n_leap; T.n_steps = n_steps; T.n_burn = n_burn; T.thin = thin; T.n_keep = n_keep;
    T.step0 = (unsigned)step0; T.k0 = (unsigned)seed; T.k1 = (unsigned)(seed >> 32);
    PerChain pc;
    pc.dH_mean = dd; pc.dH_max = dd + tot_chains;
    pc.n_accept = di; pc.n_wall = di + tot_chains; pc.status = di + 2 * tot_chains;
    hipLaunchKernelGGL(k_hmc, dim3((unsigned)tasks.size()), dim3(64 * waves), lds, st, d_grps.as<Grp>(), d_tasks.as<int2>(), T, pc);
    HIP_TRY(hipGetLastError());

    const long long sz = sizeof(double), si = sizeof(int32_t);
    if (fetch(dH_mean, pc.dH_mean, tot_chains * sz, st) || fetch(dH_max, pc.dH_max, tot_chains * sz, st) ||
        fetch(n_accept, pc.n_accept, tot_chains * si, st) || fetch(n_wall, pc.n_wall, tot_chains * si, st) ||
        fetch(chain_status, pc.status, tot_chains * si, st))
        return -1;
    for (int g = 0; g < G; ++g) {
        const Grp& R = grps[g];
        const long long keep = (long long)n_keep * R.nC, steps = (long long)n_steps * R.nC;
        if (o_chain[g] >= 0 && fetch(chain[g], R.chain, keep * R.D * sz, st)) return -1;
        if (o_last[g] >= 0 && fetch(last[g], R.last, (long long)R.nC * R.D * sz, st)) return -1;
        if (o_lnp[g] >= 0 && fetch(lnp[g], R.lnp, keep * sz, st)) return -1;
        if (o_mom[g] >= 0 && fetch(mom[g], R.mom, steps * R.D * sz, st)) return -1;
        if (o_prop[g] >= 0 && fetch(prop[g], R.prop, steps * R.D * sz, st)) return -1;
        if (o_pm[g] >= 0 && fetch(prop_mom[g], R.prop_mom, steps * R.D * sz, st)) return -1;
        if (o_dH[g] >= 0 && fetch(dH[g], R.dH, steps * sz, st)) return -1;
        if (o_acc[g] >= 0 && fetch(acc[g], R.acc, steps * si, st)) return -1;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (status)
        for (int g = 0; g < G; ++g) status[g] = st_host[g];
    return 0;
}
