// relabel.hip -- undo label switching: the optimal relabelling of the lines of ensemble chains (include/vamp_relabel.h,
// libvamp_relabel.so).  Definitions: the header, and DESIGN.md "Relabelling: undoing label switching".
//
// A sample's K lines are matched to the K lines of a reference by a K x K linear assignment problem; the reference
// then moves to the means of the relabelled samples, and the two steps repeat until no permutation changes.  The
// kernels, every one over a list of (group, first unit) tasks so that one launch serves all groups:
//   k_bad       one thread per sample: is any of its q K line parameters not finite?  One byte per sample, read by
//               every other kernel, and the group's n_bad.
//   k_assign    a group of 8, 16 or 32 lanes (from K alone) owns one sample; lane j owns reference line j.  The
//               sample's line vectors sit in LDS, a cost entry C(i, j) is q subtract-divide-square-add steps from them, so
//               no lane holds a matrix.  lap_solve below is the shortest-augmenting-path form of the Hungarian method
//               (Jonker & Volgenant): row after row is inserted, each by at most (rows so far + 1) steps of "relax my
//               column against the row just reached, group argmin over the columns outside the tree", then the
//               matching is flipped along the path found.  The argmin is a butterfly of in-group shuffles on
//               (value, column) with ties to the smaller column, so every lane of the group ends with the same pair.
//               EVERY loop of the solver has a trip count that depends on K and the row number alone: nothing runs
//               "until" a condition, the search and the walk back are switched off by a flag and the remaining trips
//               do nothing.  A sample that is bad, or whose cost matrix has an entry that is not finite, never enters
//               it: its lanes run the same instructions on a matrix of zeros (the shuffles need every lane), and the
//               result is discarded.  The one-wavefront-per-sample form was not built: 32 lanes hold K <= 32 as they
//               stand.
//   k_matrices  vamp_relabel_assign: the same lap_solve on cost matrices read from memory.
//   k_colsum    the moments, first stage: a thread owns one of the q K columns of one chunk of 64 samples and folds it
//               in sample order -- the values, or their squared distances from a centre, in place or through the
//               sample's permutation.  k_finish, one workgroup per group, folds the chunks in chunk order and turns the
//               sums into the pooled scale, the next reference, the label means or the label sds.  The chunk is fixed,
//               so no sum depends on how the tasks were packed; the counts are integer atomics, which have no order.
//   k_gather    a lane group reads its sample into LDS and writes line j <- line pi(j); reading all before writing
//               any is what makes it work in place.
// Everything is fp64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_relabel.h"
#include "relabel_host.hpp"
#include "side_call.hpp"

#define VAMP_RELABEL_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace vamp::side;
namespace rl = vamp::relabel;

constexpr int kBlock = 256;                // four wavefronts
constexpr int kMaxQ = 4;
constexpr int kLineDoubles = kBlock * kMaxQ;       // LDS of k_assign / k_gather: q K <= 4 * lanes doubles per lane group
constexpr int kFinishBlock = 128;          // q K <= 128 columns
constexpr int kNoColumn = 64;              // sorts after every column in the argmin

static_assert(rl::kMaxComponents == VAMP_RELABEL_MAX_COMPONENTS, "relabel_host.hpp checks the header's limit");
static_assert(kMaxQ * VAMP_RELABEL_MAX_COMPONENTS <= kFinishBlock && kFinishBlock <= kBlock, "a thread per column");
static_assert(rl::group_lanes(VAMP_RELABEL_MAX_COMPONENTS) == 32 && rl::group_lanes(8) == 8 && rl::group_lanes(9) == 16 &&
                  rl::group_lanes(17) == 32, "a lane group never crosses a wavefront and holds a lane per line");

struct GroupDev {
    const double* in;              // the chain, on the device
    double* out;                   // where k_gather writes; NULL: no gather for this group
    long long ld, out_ld;
    long long samp_off, perm_off, part_off;
    int col_off, sc_off;
    int W, D, K, q, S, lanes;
    int pool;                      // 1: the scale is the pooled sd
};

struct Arrays {                    // of all groups, at the offsets of GroupDev
    uint8_t* bad;                  // [tot_s]
    uint8_t* perm;                 // [tot_perm]
    double* cost;                  // [tot_s]
    double* ref;                   // [tot_col]
    double* scale;                 // [tot_sc]
    double* partial;               // [tot_part]
    int32_t* n_bad;                // [G]
    int32_t* round;                // [G][2]: n_changed, n_switched
};

enum FinishOp { kPoolMean = 0, kPoolScale = 1, kMean = 2, kSd = 3 };

__device__ __forceinline__ void lds_fence() {      // LDS traffic between the lanes of one wavefront
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// does `pred` hold on any lane of this lane's group of w lanes?
__device__ __forceinline__ bool group_any(bool pred, int w) {
    const int lane = threadIdx.x & 63;
    const unsigned long long mask = ((1ull << w) - 1ull) << ((lane / w) * w);      // w <= 32
    return (__ballot(pred) & mask) != 0ull;
}

// sample s = t W + w of a chain whose rows are ld doubles apart
__device__ __forceinline__ long long sample_off(long long ld, int W, int D, int s) {
    const int t = s / W;
    return (long long)t * ld + (long long)(s - t * W) * D;
}
__device__ __forceinline__ const double* sample_ptr(const double* base, long long ld, int W, int D, int s) {
    return base + sample_off(ld, W, D, s);
}

// The assignment of a K x K cost matrix, 2 <= K <= w, by the w lanes of a group: lane gl < K owns column gl, the
// potential v of that column and the row matched to it, and the potential u of ROW gl as well.  cost(i) is the lane's
// entry C(i, gl) (anything finite on a lane >= K).  On return `assigned` is the row given to column gl and `total`
// the sum of the assigned entries, the same on every lane.  All entries must be finite.  Finite entries so large that a
// potential or the total overflows (|C| K near DBL_MAX) can leave the search with inf - inf; the loops end all the same,
// and the return value says so: false unless `assigned` is a permutation over the group and `total` is finite.  Every
// lane of the wavefront must call this together: the trip counts depend on K alone.
template <class CostFn>
__device__ __forceinline__ bool lap_solve(int K, int w, int gl, CostFn cost, int& assigned, double& total) {
    const bool col = gl < K;
    double u = 0.0, v = 0.0;
    int p = -1;                                    // the row matched to my column; -1: free
    for (int i = 0; i < K; ++i) {                  // insert row i: a shortest augmenting path from it to a free column
        double minv = INFINITY;                    // my column's reduced distance from the tree
        int way = K;                               // the column it was reached from; K: from row i itself
        bool used = false;                         // my column is in the tree
        bool rowin = gl == i;                      // my row is in the tree
        bool searching = true;
        int i0 = i, j0 = K, jend = 0;
        for (int step = 0; step <= i; ++step) {    // i columns are matched: the (i + 1)-th reached is free at the latest
            const double cur = cost(i0) - __shfl(u, i0, w) - v;
            if (searching && col && !used && cur < minv) {
                minv = cur;
                way = j0;
            }
            double val = (col && !used) ? minv : INFINITY;
            int idx = (col && !used) ? gl : kNoColumn;
            for (int o = w >> 1; o > 0; o >>= 1) {
                const double ov = __shfl_xor(val, o, w);
                const int oi = __shfl_xor(idx, o, w);
                if (ov < val || (ov == val && oi < idx)) {
                    val = ov;
                    idx = oi;
                }
            }
            const int j1 = idx < K ? idx : K - 1;
            const int pj1 = __shfl(p, j1, w);
            if (searching) {
                if (rowin) u += val;
                if (col) {
                    if (used) v -= val;
                    else minv -= val;
                }
                if (gl == j1) used = true;
                if (pj1 < 0) {
                    searching = false;
                    jend = j1;
                } else {
                    i0 = pj1;
                    j0 = j1;
                    if (gl == i0) rowin = true;
                }
            }
        }
        int j = jend;                              // flip the matching along the path, back to row i
        bool walking = true;
        for (int step = 0; step <= i; ++step) {
            const int jw = __shfl(way, j, w);
            const int pw = __shfl(p, jw < K ? jw : 0, w);
            if (walking) {
                if (gl == j) p = jw < K ? pw : i;
                if (jw >= K) walking = false;
                else j = jw;
            }
        }
    }
    assigned = p < 0 ? 0 : (p < K ? p : K - 1);
    double c = col ? cost(assigned) : 0.0;
    unsigned seen = col ? 1u << assigned : 0u;     // K <= 32 rows
    for (int o = w >> 1; o > 0; o >>= 1) {
        c += __shfl_xor(c, o, w);
        seen |= (unsigned)__shfl_xor((int)seen, o, w);
    }
    total = c;
    return seen == (K == 32 ? ~0u : (1u << K) - 1u) && isfinite(c);
}

__global__ __launch_bounds__(kBlock) void k_bad(const GroupDev* __restrict__ groups, const int2* __restrict__ tasks, Arrays A) {
    const int2 task = tasks[blockIdx.x];
    const GroupDev G = groups[task.x];
    const long long s = (long long)task.y + threadIdx.x;
    const bool valid = s < G.S;
    bool bad = false;
    if (valid) {
        const double* p = sample_ptr(G.in, G.ld, G.W, G.D, (int)s);
        const int E = G.q * G.K;
        for (int e = 0; e < E; ++e) bad |= !isfinite(p[e]);
        A.bad[G.samp_off + s] = bad ? 1 : 0;
    }
    const int nb = __popcll(__ballot(valid && bad));
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&A.n_bad[task.x], nb);
}

__global__ __launch_bounds__(kBlock) void k_assign(const GroupDev* __restrict__ groups, const int2* __restrict__ tasks, Arrays A,
                                                   int first_round) {
    __shared__ double s_lines[kLineDoubles];
    const int2 task = tasks[blockIdx.x];
    const GroupDev G = groups[task.x];
    const int w = G.lanes, K = G.K, q = G.q, E = q * K;
    const int grp = threadIdx.x / w, gl = threadIdx.x - grp * w;
    const long long s = (long long)task.y + grp;
    const bool valid = s < G.S;
    const bool live = valid && !A.bad[G.samp_off + (valid ? s : 0)];
    double* sv = s_lines + grp * (kMaxQ * w);
    if (valid) {
        const double* p = sample_ptr(G.in, G.ld, G.W, G.D, (int)s);
        for (int e = gl; e < E; e += w) sv[e] = p[e];
    } else {
        for (int e = gl; e < E; e += w) sv[e] = 0.0;
    }
    lds_fence();

    const bool col = gl < K;
    double rj[kMaxQ], sc[kMaxQ];
#pragma unroll
    for (int d = 0; d < kMaxQ; ++d) {
        rj[d] = (col && d < q) ? A.ref[G.col_off + gl * q + d] : 0.0;
        sc[d] = d < q ? A.scale[G.sc_off + d] : 1.0;
    }
    auto entry = [&](int i) {                      // C(i, gl), summed in d order; every step rounded once, as the definition reads
#pragma clang fp contract(off)
        double c = 0.0;
#pragma unroll
        for (int d = 0; d < kMaxQ; ++d)
            if (d < q) {
                const double t = (sv[i * q + d] - rj[d]) / sc[d];
                c = c + t * t;                 // (no fma: the pragma above)
            }
        return c;
    };

    bool finite = true;
    if (live && col)
        for (int i = 0; i < K; ++i) finite &= isfinite(entry(i)) != 0;
    const bool solve = live && !group_any(live && col && !finite, w);
    int pj = gl;
    double tot = NAN;
    if (K == 1) {
        if (solve) tot = entry(0);
    } else if (__ballot(solve) != 0ull) {          // wavefront-uniform
        int got;
        double sum;
        const bool ok = lap_solve(K, w, gl, [&](int i) { return (solve && col) ? entry(i) : 0.0; }, got, sum);
        if (solve && ok) {                         // an overflow inside the solver: as a matrix that is not finite
            pj = got;
            tot = sum;
        }
    }

    bool changed = false, switched = false;
    if (valid && col) {
        uint8_t* dst = A.perm + G.perm_off + s * K + gl;
        const int prev = first_round ? gl : (int)*dst;
        changed = live && pj != prev;
        switched = live && pj != gl;
        *dst = (uint8_t)pj;
    }
    changed = group_any(changed, w);
    switched = group_any(switched, w);
    if (valid && gl == 0) A.cost[G.samp_off + s] = tot;
    const int nc = __popcll(__ballot(gl == 0 && changed)), ns = __popcll(__ballot(gl == 0 && switched));
    if ((threadIdx.x & 63) == 0) {
        if (nc) atomicAdd(&A.round[2 * task.x], nc);
        if (ns) atomicAdd(&A.round[2 * task.x + 1], ns);
    }
}

// vamp_relabel_assign: matrix m is cost[m K K ..], row-major C(i, j)
__global__ __launch_bounds__(kBlock) void k_matrices(const double* __restrict__ cost, int K, int n, int w, uint8_t* __restrict__ perm,
                                                     double* __restrict__ total) {
    const int grp = threadIdx.x / w, gl = threadIdx.x - grp * w;
    const long long m = (long long)blockIdx.x * (kBlock / w) + grp;
    const bool valid = m < n, col = gl < K;
    const double* c = cost + (valid ? m : 0) * K * K;
    bool finite = true;
    if (valid && col)
        for (int i = 0; i < K; ++i) finite &= isfinite(c[i * K + gl]) != 0;
    const bool solve = valid && !group_any(valid && col && !finite, w);
    int pj = gl;
    double tot = NAN;
    if (K == 1) {
        if (solve) tot = c[0];
    } else if (__ballot(solve) != 0ull) {
        int got;
        double sum;
        const bool ok = lap_solve(K, w, gl, [&](int i) { return (solve && col) ? c[i * K + gl] : 0.0; }, got, sum);
        if (solve && ok) {
            pj = got;
            tot = sum;
        }
    }
    if (valid && col) perm[m * K + gl] = (uint8_t)pj;
    if (valid && gl == 0) total[m] = tot;
}

// first stage of the moments: partial[chunk][e] = sum over the chunk's good samples, in sample order, of column e of
// the (relabelled, if use_perm) sample, or of its squared distance from centre[e]
__global__ __launch_bounds__(kBlock) void k_colsum(const GroupDev* __restrict__ groups, const int2* __restrict__ tasks, Arrays A,
                                                   int use_perm, const double* __restrict__ centre) {
    const int2 task = tasks[blockIdx.x];
    const GroupDev G = groups[task.x];
    const int E = G.q * G.K;
    const int sub = threadIdx.x / E, e = threadIdx.x - sub * E;
    const long long chunk = (long long)task.y + sub;
    if (sub >= kBlock / E || chunk >= rl::n_chunks(G.S)) return;
    const int j = e / G.q, d = e - j * G.q;
    const double c = centre ? centre[G.col_off + e] : 0.0;
    const long long s0 = chunk * rl::kChunk, s1 = s0 + rl::kChunk < G.S ? s0 + rl::kChunk : G.S;
    double acc = 0.0;
    for (long long s = s0; s < s1; ++s) {
        if (A.bad[G.samp_off + s]) continue;
        const int src = use_perm ? (int)A.perm[G.perm_off + s * G.K + j] * G.q + d : e;
        const double x = sample_ptr(G.in, G.ld, G.W, G.D, (int)s)[src];
        acc += centre ? (x - c) * (x - c) : x;
    }
    A.partial[G.part_off + chunk * E + e] = acc;
}

// second stage: the chunks in chunk order, then what `op` makes of the column totals of the n good samples
__global__ __launch_bounds__(kFinishBlock) void k_finish(const GroupDev* __restrict__ groups, Arrays A, int op, double* __restrict__ dst) {
    __shared__ double s_tot[kFinishBlock];
    const GroupDev G = groups[blockIdx.x];
    const int E = G.q * G.K, e = threadIdx.x;
    if ((op == kPoolMean || op == kPoolScale) && !G.pool) return;
    double tot = 0.0;
    if (e < E) {
        const long long nch = rl::n_chunks(G.S);
        const double* part = A.partial + G.part_off + e;
        for (long long c = 0; c < nch; ++c) tot += part[c * E];
    }
    s_tot[e] = tot;
    __syncthreads();
    const double n = (double)(G.S - A.n_bad[blockIdx.x]);
    if (op == kPoolMean || op == kPoolScale) {     // pooled over the K lines, in line order
        if (e >= E) return;
        const int d = e % G.q;
        double sum = 0.0;
        for (int j = 0; j < G.K; ++j) sum += s_tot[j * G.q + d];
        const double m = G.K * n;
        if (op == kPoolMean) {
            dst[G.col_off + e] = sum / m;          // the centre of every line's column d
        } else if (e < G.q) {
            double sd = sqrt(sum / (m - 1.0));
            if (!(m >= 2.0) || !(sd > 0.0) || !isfinite(sd)) sd = 1.0;
            dst[G.sc_off + d] = sd;
        }
    } else if (e < E) {
        if (op == kMean) dst[G.col_off + e] = tot / n;                     // n = 0: NaN
        else dst[G.col_off + e] = n >= 2.0 ? sqrt(tot / (n - 1.0)) : NAN;
    }
}

__global__ __launch_bounds__(kBlock) void k_gather(const GroupDev* __restrict__ groups, const int2* __restrict__ tasks, Arrays A) {
    __shared__ double s_lines[kLineDoubles];
    const int2 task = tasks[blockIdx.x];
    const GroupDev G = groups[task.x];
    const int w = G.lanes, K = G.K, q = G.q, E = q * K;
    const int grp = threadIdx.x / w, gl = threadIdx.x - grp * w;
    const long long s = (long long)task.y + grp;
    const bool valid = s < G.S;
    double* sv = s_lines + grp * (kMaxQ * w);
    const double* src = valid ? sample_ptr(G.in, G.ld, G.W, G.D, (int)s) : nullptr;
    double sd = 0.0;
    if (valid) {
        for (int e = gl; e < E; e += w) sv[e] = src[e];
        if (gl == 0 && G.D > E) sd = src[E];
    }
    lds_fence();                                   // the whole sample is read before any of it is written
    if (!valid) return;
    double* dst = G.out + sample_off(G.out_ld, G.W, G.D, (int)s);
    const uint8_t* pi = A.perm + G.perm_off + s * K;
    for (int e = gl; e < E; e += w) {
        const int j = e / q, d = e - j * q;
        dst[e] = sv[(int)pi[j] * q + d];
    }
    if (gl == 0 && G.D > E && dst != src) dst[E] = sd;
}

template <class T>
std::vector<int2> as_int2(const std::vector<T>& tasks) {
    std::vector<int2> v;
    v.reserve(tasks.size());
    for (const T& t : tasks) v.push_back(make_int2(t.group, t.first));
    return v;
}

}  // namespace

VAMP_RELABEL_API int vamp_relabel_version(void) { return VAMP_RELABEL_ABI_VERSION; }

VAMP_RELABEL_API const char* vamp_relabel_last_error(void) { return g_err.c_str(); }

VAMP_RELABEL_API int vamp_relabel_chains(int device, void* hip_stream, int n_groups, const int32_t* n_comp, const int32_t* mode,
                                         const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                                         const int32_t* n_keep, const int32_t* walkers, const double* const* ref,
                                         const double* const* scale, int max_iter, double* const* out, const int64_t* out_ld,
                                         int out_is_device, uint8_t* const* perm, double* const* cost, double* label_mean,
                                         double* label_sd, double* scale_used, int32_t* n_iter, int32_t* n_changed,
                                         int32_t* n_switched, int32_t* n_used, int32_t* n_bad) {
    g_err.clear();
    const std::string fn = "vamp_relabel_chains: ";
    if (n_groups <= 0) return fail(fn + "n_groups must be positive");
    if (!n_comp || !mode || !sample_sd || !base || !ld || !n_keep || !walkers || !ref) return fail(fn + "NULL argument");
    rl::Groups rg;
    const std::string err = rl::check_groups(fn, n_groups, n_comp, mode, sample_sd, base, is_device, ld, n_keep, walkers, ref, scale,
                                             max_iter, out, out_ld, out_is_device, rg);
    if (!err.empty()) return fail(err);
    const int G = n_groups;

    // tasks: samples per workgroup of k_bad (a thread each) and of k_assign / k_gather (a lane group each), chunks of k_colsum
    std::vector<long long> n_samp(G), n_chunk(G), n_pool(G), n_gather(G);
    std::vector<int> per_thread(G, kBlock), per_group(G), per_sub(G);
    bool any_pool = false, any_out = false;
    for (int g = 0; g < G; ++g) {
        n_samp[g] = rg.S[g];
        n_chunk[g] = rl::n_chunks(rg.S[g]);
        n_gather[g] = (out && out[g]) ? rg.S[g] : 0;
        per_group[g] = kBlock / rg.lanes[g];
        per_sub[g] = kBlock / (rg.q[g] * n_comp[g]);
        n_pool[g] = (scale && scale[g]) ? 0 : n_chunk[g];            // the pooled scale is summed for the groups that ask for it
        any_pool |= n_pool[g] != 0;
        any_out |= n_gather[g] != 0;
    }
    const std::vector<int2> t_bad = as_int2(rl::plan_tasks(n_samp, per_thread)), t_assign = as_int2(rl::plan_tasks(n_samp, per_group)),
                            t_sum = as_int2(rl::plan_tasks(n_chunk, per_sub)), t_pool = as_int2(rl::plan_tasks(n_pool, per_sub)),
                            t_gather = as_int2(rl::plan_tasks(n_gather, per_group));
    if (t_assign.size() > 0x7fffffff) return fail(fn + "too many workgroups");

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    // device view of every group's chain: staged (host input) or as given
    std::vector<const double*> dbase(base, base + G);
    DevBuf staging, out_tmp;
    if (!is_device) {
        std::vector<long long> len(G);
        for (int g = 0; g < G; ++g) len[g] = chain_span(n_keep[g], ld[g], walkers[g], rg.D[g]);
        if (stage_chains(len, base, st, staging, dbase)) return -1;
    }
    // where k_gather writes: the caller's device chain; or, for a host `out`, the staged copy itself (in place: the
    // copy is this call's own) or, when the input is the caller's device chain, a compact buffer
    std::vector<double*> dout(G, nullptr);
    std::vector<long long> dout_ld(G, 0);
    if (any_out) {
        long long tmp_len = 0;
        for (int g = 0; g < G; ++g)
            if (out[g] && !out_is_device && is_device) tmp_len += (long long)rg.S[g] * rg.D[g];
        if (tmp_len) HIP_TRY(hipMalloc(&out_tmp.p, (size_t)tmp_len * sizeof(double)));
        long long off = 0;
        for (int g = 0; g < G; ++g) {
            if (!out[g]) continue;
            if (out_is_device) {
                dout[g] = out[g];
                dout_ld[g] = out_ld[g];
            } else if (!is_device) {
                dout[g] = const_cast<double*>(dbase[g]);
                dout_ld[g] = ld[g];
            } else {
                dout[g] = out_tmp.as<double>() + off;
                dout_ld[g] = (long long)walkers[g] * rg.D[g];
                off += (long long)rg.S[g] * rg.D[g];
            }
        }
    }

    std::vector<GroupDev> groups(G);
    std::vector<double> h_ref((size_t)rg.tot_col), h_scale((size_t)rg.tot_sc, 1.0);
    for (int g = 0; g < G; ++g) {
        GroupDev& d = groups[g];
        d.in = dbase[g];
        d.out = dout[g];
        d.ld = ld[g];
        d.out_ld = dout_ld[g];
        d.samp_off = rg.samp_off[g]; d.perm_off = rg.perm_off[g]; d.part_off = rg.part_off[g];
        d.col_off = rg.col_off[g]; d.sc_off = rg.sc_off[g];
        d.W = walkers[g]; d.D = rg.D[g]; d.K = n_comp[g]; d.q = rg.q[g]; d.S = rg.S[g]; d.lanes = rg.lanes[g];
        d.pool = !(scale && scale[g]);
        for (int e = 0; e < d.q * d.K; ++e) h_ref[d.col_off + e] = ref[g][e];
        if (!d.pool)
            for (int e = 0; e < d.q; ++e) h_scale[d.sc_off + e] = scale[g][e];
    }

    DevBuf d_groups, d_tbad, d_tassign, d_tsum, d_tpool, d_tgather, d_bad, d_perm, d_cost, d_ref, d_scale, d_partial, d_mean, d_sd, d_nbad, d_round;
    if (upload(d_groups, groups, st) || upload(d_tbad, t_bad, st) || upload(d_tassign, t_assign, st) || upload(d_tsum, t_sum, st) || upload(d_tpool, t_pool, st) ||
        upload(d_tgather, t_gather, st) || upload(d_ref, h_ref, st) || upload(d_scale, h_scale, st))
        return -1;
    HIP_TRY(hipMalloc(&d_bad.p, (size_t)rg.tot_s));
    HIP_TRY(hipMalloc(&d_perm.p, (size_t)rg.tot_perm));
    HIP_TRY(hipMalloc(&d_cost.p, (size_t)rg.tot_s * sizeof(double)));
    HIP_TRY(hipMalloc(&d_partial.p, (size_t)rg.tot_part * sizeof(double)));
    HIP_TRY(hipMalloc(&d_mean.p, (size_t)rg.tot_col * sizeof(double)));
    HIP_TRY(hipMalloc(&d_sd.p, (size_t)rg.tot_col * sizeof(double)));
    HIP_TRY(hipMalloc(&d_nbad.p, (size_t)G * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&d_round.p, (size_t)G * 2 * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(d_nbad.p, 0, (size_t)G * sizeof(int32_t), st));
    const Arrays A{d_bad.as<uint8_t>(), d_perm.as<uint8_t>(), d_cost.as<double>(), d_ref.as<double>(), d_scale.as<double>(),
                   d_partial.as<double>(), d_nbad.as<int32_t>(), d_round.as<int32_t>()};
    const GroupDev* dg = d_groups.as<GroupDev>();

    // the moments of the (relabelled) columns about `centre` (NULL: the plain sums), finished by `op` into `dst`; the
    // pooled passes run over the groups without a given scale only
    auto moments = [&](int use_perm, const double* centre, int op, double* dst) -> int {
        const bool pooled = op == kPoolMean || op == kPoolScale;
        const std::vector<int2>& tasks = pooled ? t_pool : t_sum;
        hipLaunchKernelGGL(k_colsum, dim3((unsigned)tasks.size()), dim3(kBlock), 0, st, dg, (pooled ? d_tpool : d_tsum).as<int2>(), A, use_perm,
                           centre);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_finish, dim3((unsigned)G), dim3(kFinishBlock), 0, st, dg, A, op, dst);
        HIP_TRY(hipGetLastError());
        return 0;
    };

    hipLaunchKernelGGL(k_bad, dim3((unsigned)t_bad.size()), dim3(kBlock), 0, st, dg, d_tbad.as<int2>(), A);
    HIP_TRY(hipGetLastError());
    if (any_pool) {                                // d_mean holds the pooled centres until the first round needs it
        if (moments(0, nullptr, kPoolMean, d_mean.as<double>()) || moments(0, d_mean.as<double>(), kPoolScale, d_scale.as<double>()))
            return -1;
    }

    std::vector<int32_t> h_round((size_t)G * 2), iters(G, 0);
    int r = 1;
    for (;; ++r) {
        HIP_TRY(hipMemsetAsync(d_round.p, 0, (size_t)G * 2 * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_assign, dim3((unsigned)t_assign.size()), dim3(kBlock), 0, st, dg, d_tassign.as<int2>(), A, r == 1 ? 1 : 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_round.data(), d_round.p, h_round.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool all_done = r > 1;
        for (int g = 0; g < G; ++g) {
            if (!iters[g] && r > 1 && h_round[2 * g] == 0) iters[g] = r;
            all_done &= iters[g] != 0;
        }
        if (all_done || r == max_iter) break;
        if (moments(1, nullptr, kMean, d_ref.as<double>())) return -1;       // the next round's reference
    }
    for (int g = 0; g < G; ++g)
        if (!iters[g]) iters[g] = r;

    if (label_mean || label_sd) {
        if (moments(1, nullptr, kMean, d_mean.as<double>()) || moments(1, d_mean.as<double>(), kSd, d_sd.as<double>())) return -1;
    }
    if (any_out) {                                 // last: in place it overwrites what the moments read
        hipLaunchKernelGGL(k_gather, dim3((unsigned)t_gather.size()), dim3(kBlock), 0, st, dg, d_tgather.as<int2>(), A);
        HIP_TRY(hipGetLastError());
        for (int g = 0; g < G && !out_is_device; ++g) {
            if (!out[g]) continue;
            const size_t row = (size_t)walkers[g] * rg.D[g] * sizeof(double);
            HIP_TRY(hipMemcpy2DAsync(out[g], (size_t)out_ld[g] * sizeof(double), dout[g], (size_t)dout_ld[g] * sizeof(double), row,
                                     (size_t)n_keep[g], hipMemcpyDeviceToHost, st));
        }
    }
    for (int g = 0; g < G; ++g) {
        if (perm && fetch(perm[g], d_perm.as<uint8_t>() + rg.perm_off[g], (long long)rg.S[g] * n_comp[g], st)) return -1;
        if (cost && fetch(cost[g], d_cost.as<double>() + rg.samp_off[g], (long long)rg.S[g] * sizeof(double), st)) return -1;
    }
    std::vector<int32_t> h_bad(G);
    if (fetch(label_mean, d_mean.p, rg.tot_col * (long long)sizeof(double), st) ||
        fetch(label_sd, d_sd.p, rg.tot_col * (long long)sizeof(double), st) ||
        fetch(scale_used, d_scale.p, rg.tot_sc * (long long)sizeof(double), st) ||
        fetch(h_bad.data(), d_nbad.p, G * (long long)sizeof(int32_t), st))
        return -1;
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < G; ++g) {
        if (n_iter) n_iter[g] = iters[g];
        if (n_changed) n_changed[g] = h_round[2 * g];
        if (n_switched) n_switched[g] = h_round[2 * g + 1];
        if (n_used) n_used[g] = rg.S[g] - h_bad[g];
        if (n_bad) n_bad[g] = h_bad[g];
    }
    return 0;
}

VAMP_RELABEL_API int vamp_relabel_assign(int device, int K, int n, const double* cost, uint8_t* perm, double* total) {
    g_err.clear();
    const std::string fn = "vamp_relabel_assign: ";
    const std::string err = rl::check_assign(fn, K, n, cost);
    if (!err.empty()) return fail(err);
    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = nullptr;
    const size_t len = (size_t)n * K * K;
    DevBuf d_cost, d_perm, d_total;
    HIP_TRY(hipMalloc(&d_cost.p, len * sizeof(double)));
    HIP_TRY(hipMalloc(&d_perm.p, (size_t)n * K));
    HIP_TRY(hipMalloc(&d_total.p, (size_t)n * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(d_cost.p, cost, len * sizeof(double), hipMemcpyHostToDevice, st));
    const int w = rl::group_lanes(K), per_block = kBlock / w;
    hipLaunchKernelGGL(k_matrices, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kBlock), 0, st, d_cost.as<double>(), K, n, w,
                       d_perm.as<uint8_t>(), d_total.as<double>());
    HIP_TRY(hipGetLastError());
    if (fetch(perm, d_perm.p, (long long)n * K, st) || fetch(total, d_total.p, n * (long long)sizeof(double), st)) return -1;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
