// lane_group.hpp -- a group of lanes that owns one parameter vector: what k_post_eval (posterior.hip), k_pointwise_ll
// (pointwise_ll.hpp) and eval_point (evidence.hip) share.  A wavefront -- or, for short regions of few lines, a 16-lane
// group -- turns the vector into line records once (centre, scale, damping, amplitude factor, pole factor, h y:
// line_record below is the record of a chain's sample; the evidence's builder differs and stays in its file), fills
// the 44-entry near-axis table of every Voigt line (voigt_math.hpp) in LDS, then its lanes walk the pixels.  Also
// the workgroup reductions of fixed order.
#pragma once

#include <hip/hip_runtime.h>

#include "voigt_math.hpp"

namespace vamp {

constexpr int kNarrowLanes = 16, kNarrowMaxPix = 32, kNarrowMaxK = 4;

// lanes that own a vector of K lines on P pixels: 64 or kNarrowLanes.  `narrow`: the library's switch
// (VAMP_POST_NARROW, VAMP_PRED_NARROW, VAMP_EVID_NARROW)
__host__ __device__ constexpr int group_lanes(bool narrow, int P, int K) {
    return (narrow && P <= kNarrowMaxPix && K <= kNarrowMaxK) ? kNarrowLanes : 64;
}

struct LaneGroup {
    int nsub;                      // groups in a wavefront
    int sub, gl;                   // the lane's group, and its index in the group
};

__device__ __forceinline__ LaneGroup lane_group(int lane, int lanes) {
    LaneGroup g;
    g.nsub = 64 / lanes;
    g.sub = lane / lanes;
    g.gl = lane - g.sub * lanes;
    return g;
}

// the ballot bits of group `sub` of `lanes` lanes: one bad lane makes its group's sample bad, and no other's
__device__ __forceinline__ unsigned long long group_mask(int lanes, int sub) {
    return (lanes == 64 ? ~0ull : ((1ull << lanes) - 1ull)) << (sub * lanes);
}

// The record r[0 .. 5] of one line of a chain's sample from its parameters th -- (A, c, L_fwhm, G_fwhm), or (A, c,
// sigma) -- and whether they make the sample bad: one that is not finite, or sigma <= 0, or G <= 0, or L < 0.
__device__ __forceinline__ bool line_record(bool voigt, const double* th, double* r) {
    constexpr double SQRT_LN2 = 0.83255461115769775635;
    const double a = th[0], c = th[1];
    bool bad;
    r[0] = c;
    if (voigt) {
        const double Lw = th[2], G = th[3];
        bad = !(isfinite(a) && isfinite(c) && isfinite(Lw) && isfinite(G)) || G <= 0.0 || Lw < 0.0;
        const double rG = rcp_nr(G);
        const double y = (Lw * SQRT_LN2) * rG;
        r[1] = (2.0 * SQRT_LN2) * rG;
        r[2] = y;
        r[3] = a * y;                      // tau_k = A y sqrt(pi) H: the evaluator returns sqrt(pi) H
        r[4] = core_pole_factor(y);
        r[5] = core_hy(y);
    } else {
        const double sg = th[2];
        bad = !(isfinite(a) && isfinite(c) && isfinite(sg)) || sg <= 0.0;
        r[1] = 1.0 / sg; r[2] = 0.0; r[3] = a; r[4] = 0.0; r[5] = 0.0;
    }
    return bad;
}

__device__ __forceinline__ void lds_fence() {      // LDS traffic between the lanes of one wavefront
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the near-axis tables of K lines, by the group's lanes; the damping y is entry 2 of a record of REC doubles
template <int REC>
__device__ __forceinline__ void fill_dtab(double* dtab, const double* rec, int K, int gl, int lanes) {
    for (int e = gl; e < K * DTAB_N; e += lanes) {
        const int k = e / DTAB_N, n = e - k * DTAB_N;
        dtab[e] = core_dtab_entry(n, rec[k * REC + 2]);
    }
}

// optical depth of one line at x from its record r (centre, scale, damping, amplitude factor, pole factor, h y)
__device__ __forceinline__ double line_tau(bool voigt, double x, const double* r, const double* dtab_k) {
    if (voigt) return r[3] * voigt_Hs(fabs(x - r[0]) * r[1], r[2], dtab_k, r[4], r[5]);
    const double u = (x - r[0]) * r[1];
    return r[3] * exp(-0.5 * (u * u));
}

// sum / maximum over a workgroup of BLOCK threads in a fixed order; red: BLOCK doubles of LDS
template <int BLOCK>
__device__ inline double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
template <int BLOCK>
__device__ inline double block_max(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

}  // namespace vamp
