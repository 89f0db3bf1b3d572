// pointwise_ll.hpp -- the pointwise log-likelihood stage of predictive.hip and loo.hip: l_sp, the log-likelihood of
// pixel p's datum under sample s of a group's chain, written to the scratch matrix of an item (group, pixel range).
// Both model-comparison criteria (WAIC, PSIS-LOO) rest on this one quantity, so it is defined once: the item, the
// evaluation kernel, the walk over the plan that builds items and tasks, and the launch of a pass.  DESIGN.md
// "Pointwise predictive density and WAIC".
//
//   k_pointwise_ll  one workgroup per (item, 64 samples).  A wavefront -- or, for short regions of few lines, a
//                   16-lane group -- owns a sample: its parameters become line records and near-axis tables in LDS
//                   once (lane_group.hpp), then its lanes walk the item's pixels and write l_sp.  kPixelMajor is the
//                   orientation of the scratch: ll[p * S + s] (true) or ll[s * np + p] (false).
// The largest launch (32 lines, four wavefronts) takes 51 200 bytes of LDS.  Everything is fp64.
//
// Each library is one translation unit and both code objects may be loaded into one process: the kernel has internal
// linkage, so the libraries share its source and not its symbol.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "chain_groups.hpp"
#include "lane_group.hpp"
#include "side_call.hpp"
#include "voigt_math.hpp"

namespace vamp {
namespace side {

constexpr int kEvalBlock = 256;            // four wavefronts
constexpr int kEvalWaves = kEvalBlock / 64;
constexpr int kSamplesPerBlock = 64;
constexpr int kRec = 6;                    // doubles of a line record
constexpr int kEvalMaxComponents = 32;     // VAMP_PRED_MAX_COMPONENTS, VAMP_LOO_MAX_COMPONENTS
constexpr double HALF_LN_2PI = 0.91893853320467274178;

// LDS of one sample: line records and near-axis tables
__host__ __device__ constexpr int slot_doubles(int K) { return K * (kRec + vamp::DTAB_N); }
static_assert((size_t)kEvalWaves * slot_doubles(kEvalMaxComponents) * sizeof(double) <= 64 * 1024 &&
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
    int W, D, K, q;                // q = 3 (Gauss) or 4 (Voigt) parameters per line
    int S, np, lanes;              // lanes that own a sample (vamp::group_lanes)
};

namespace {

template <bool kPixelMajor>
__global__ __launch_bounds__(kEvalBlock) void k_pointwise_ll(const Item* __restrict__ items, const int2* __restrict__ tasks,
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
    const unsigned long long gmask = vamp::group_mask(lanes, sub);

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
            if (gl < K) bad_lane |= vamp::line_record(voigt, th + I.q * gl, rec + gl * kRec);
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
            double* out = I.ll + (kPixelMajor ? (long long)s : (long long)s * I.np);
            for (int p = gl; p < I.np; p += lanes) {
                const double xi = I.x[p];
                double tau = 0.0;
                for (int k = 0; k < K; ++k) tau += vamp::line_tau(voigt, xi, rec + k * kRec, dtab + k * vamp::DTAB_N);
                const double sigma = free_sd ? sd : I.noise[p], ln_sigma = free_sd ? ln_sd : I.ln_noise[p];
                const double r = (I.y[p] - exp(-tau)) / sigma;
                out[(long long)p * (kPixelMajor ? I.S : 1)] = -0.5 * (r * r) - ln_sigma - HALF_LN_2PI;
            }
        }
        lds_fence();                                   // the records are free for the next sample
    }
}

}  // namespace

// One item per range of the plan, one task per (item, 64 samples), and of every pass (a struct with etask0, etask1 and
// region_doubles) its tasks and the LDS of a wavefront.  `in`: the device copy of pack_chain_data's vector, laid out
// as `off`; `scratch`, `bad`: the pass scratch and the [tot_s] flags; `narrow`: a 16-lane group may own a sample.
template <class Pass>
void build_eval(const PassPlan& plan, const ChainGroups& cg, const DataOffsets& off, const double* in, const double* const* noise,
                const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode, const int64_t* ld, const int32_t* walkers,
                const std::vector<const double*>& dbase, bool narrow, double* scratch, uint8_t* bad, std::vector<Item>& items,
                std::vector<int2>& etasks, std::vector<Pass>& passes) {
    long long pix_off = 0, noise_off = 0, s_off = 0;     // of the range's group
    for (const Range& r : plan.ranges) {
        const int g = r.group, S = cg.S[g], K = n_comp[g], P = n_pix[g], p0 = r.p0;
        const int lanes = vamp::group_lanes(narrow, P, K);
        const int region = (64 / lanes) * slot_doubles(K);
        Pass& ps = passes[r.pass];
        if (r.offset == 0) ps.etask0 = etasks.size();
        Item it;
        it.chain = dbase[g];
        it.x = in + off.x + pix_off + p0;
        it.y = in + off.y + pix_off + p0;
        it.noise = noise[g] ? in + off.noise + noise_off + p0 : nullptr;
        it.ln_noise = noise[g] ? in + off.ln_noise + noise_off + p0 : nullptr;
        it.ll = scratch + r.offset;
        it.bad = bad + s_off;
        it.ld = ld[g];
        it.W = walkers[g]; it.D = cg.D[g]; it.K = K; it.q = mode[g] == 1 ? 4 : 3;
        it.S = S; it.np = r.np; it.lanes = lanes;
        const int ii = (int)items.size();
        items.push_back(it);
        for (int s0 = 0; s0 < S; s0 += kSamplesPerBlock) etasks.push_back(make_int2(ii, s0));
        ps.region_doubles = region > ps.region_doubles ? region : ps.region_doubles;
        ps.etask1 = etasks.size();
        if (p0 + r.np == P) { pix_off += P; noise_off += noise[g] ? P : 0; s_off += S; }
    }
}

// the evaluation of a pass
template <bool kPixelMajor, class Pass>
int launch_eval(const Pass& ps, const DevBuf& d_items, const DevBuf& d_etasks, hipStream_t st) {
    hipLaunchKernelGGL(k_pointwise_ll<kPixelMajor>, dim3((unsigned)(ps.etask1 - ps.etask0)), dim3(kEvalBlock),
                       (size_t)kEvalWaves * ps.region_doubles * sizeof(double), st, d_items.as<Item>(),
                       d_etasks.as<int2>() + ps.etask0, ps.region_doubles);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace side
}  // namespace vamp
