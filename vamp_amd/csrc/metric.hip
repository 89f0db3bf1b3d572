// metric.hip -- a positive-definite metric from any symmetric matrix: eigen-decomposition in prior units by cyclic
// two-sided Jacobi, eigenvalues clamped, covariance, precision, ln det and Cholesky factor (include/vamp_metric.h,
// libvamp_metric.so).  Definitions: the header, and DESIGN.md section 18.
//
// A call is one launch of k_metric.  One 64-lane wavefront owns one matrix; up to four matrices share a workgroup (fewer
// when the call's largest D would not leave them room in LDS).  A and V stay in the wavefront's dynamic LDS for the whole
// decomposition, rows kRowStride(D) = n + 1 doubles apart (n = D rounded up to even): odd, so a lane per row at one
// column and a lane per column at one row are both free of bank conflicts.  The wavefronts of a workgroup finish in
// different sweeps, so the kernel has no workgroup barrier at all: only lds_fence() orders a wavefront's own LDS traffic.
//   1. the scaled matrix B into A, I into V; the Frobenius norm in a fixed order; a bad entry ends here (status 2)
//   2. sweeps of n - 1 rounds: lanes 0 .. n/2 - 1 compute their pair's (c, s) from the matrix as it stands; then a lane
//      owns a column for the row update, a row for the column update and for V (two passes when n > 64); the pair's
//      lane zeroes a_pq and a_qp.  A wavefront-wide vote after a sweep ends the loop when no pair rotated.
//   3. the diagonal sorted by rank counting; lam, the clamps and their counts
//   4. cov and prec, the lower triangle dealt over the lanes, each entry an fma chain in sorted order; ln det
//   5. the wavefront factorises the scaled cov as fisher.hip does (a lane per row); chol
// Every loop has a trip count fixed before the launch but the sweep loop's early exit.  Everything is fp64; results
// leave the kernel by ordinary vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_metric.h"
#include "lane_group.hpp"
#include "metric_host.hpp"
#include "side_call.hpp"

#define VAMP_METRIC_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace vamp::side;
using namespace vamp::metric;
using vamp::lds_fence;

static_assert(kMaxDim == VAMP_METRIC_MAX_DIM && kMaxSweeps == VAMP_METRIC_MAX_SWEEPS && kMaxMatrixDoubles == VAMP_METRIC_MAX_MATRIX_DOUBLES,
              "metric_host.hpp restates the header's limits");

struct Task {                      // one matrix
    const double* a;               // device: its entry (0, 0)
    long long ld;
    long long o_vec, o_mat, o_pt;  // where its results stand in the outputs
    long long o_scale;             // its group's scales
    double lam_lo, lam_hi;
    int D, kind;
};

struct Out {
    double *eig, *vec, *cov, *prec, *chol, *logdet, *off;
    int32_t *n_low, *n_high, *sweeps, *status;
};

// entry e of a lower triangle stored row by row: e = i (i + 1) / 2 + j, j <= i
__device__ __forceinline__ void tri_index(int e, int& i, int& j) {
    i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > e) --i;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    j = e - i * (i + 1) / 2;
}

__device__ __forceinline__ void fill(double* dst, long long n, double v, int lane) {
    for (long long e = lane; e < n; e += 64) dst[e] = v;
}

// Dynamic LDS: one slot of `slot` doubles per wavefront
__global__ __launch_bounds__(64 * kMaxWaves) void k_metric(const Task* __restrict__ tasks, long long n_tasks, const double* __restrict__ scales,
                                                           int n_sweeps, int slot, Out out) {
    extern __shared__ double lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long ti = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    if (ti >= n_tasks) return;                     // (no barrier follows: a wavefront is on its own from the start)
    const Task T = tasks[ti];
    const int D = T.D, n = padded(D), ls = row_stride(D), half = n >> 1, DD = D * D;
    double* A = lds + (size_t)wave * slot;
    double* V = A + n * ls;
    double* cs = V + n * ls;       // (c, s) of pair k at 2 k
    double* dg = cs + n;           // the diagonal
    double* sc = dg + n;           // the scales
    double* w = sc + n;            // lam~ in sorted order
    double* iw = w + n;            // the row sums of the norm; then 1 / lam~
    double* sq = iw + n;           // sqrt(cov_aa)
    int* pq = reinterpret_cast<int*>(sq + n);      // (p, q) of pair k at 2 k
    int* ord = pq + n;             // the slot of the i-th eigenvalue

    double* o_eig = out.eig + T.o_vec;
    double* o_vecs = out.vec + T.o_mat;
    double* o_cov = out.cov + T.o_mat;
    double* o_prec = out.prec + T.o_mat;
    double* o_chol = out.chol + T.o_mat;

    // 1. the scaled matrix, the identity, the norm
    for (int d = lane; d < n; d += 64) sc[d] = d < D ? scales[T.o_scale + d] : 1.0;
    lds_fence();
    bool bad = false;
    for (int e = lane; e < n * n; e += 64) {
        const int i = e / n, j = e - i * n;
        double v = 0.0;
        if (i < D && j < D) {
            const int hi = max(i, j), lo = min(i, j);
            const double h = T.a[(long long)hi * T.ld + lo];
            v = T.kind == 0 ? (sc[hi] * h) * sc[lo] : h / (sc[hi] * sc[lo]);
            bad = bad || !isfinite(h) || !isfinite(v);
        }
        A[i * ls + j] = v;
        V[i * ls + j] = i == j ? 1.0 : 0.0;
    }
    lds_fence();
    for (int i = lane; i < n; i += 64) {
        double r = 0.0;
        for (int j = 0; j < D; ++j) r = fma(A[i * ls + j], A[i * ls + j], r);
        iw[i] = r;
    }
    lds_fence();
    double norm2 = 0.0;
    for (int i = 0; i < D; ++i) norm2 += iw[i];
    const double tol = 0x1p-52 * sqrt(norm2);
    bad = bad || !isfinite(tol);
    if (__any(bad ? 1 : 0)) {                      // (uniform) status 2
        fill(o_eig, D, NAN, lane);
        fill(o_vecs, DD, NAN, lane); fill(o_cov, DD, NAN, lane); fill(o_prec, DD, NAN, lane); fill(o_chol, DD, NAN, lane);
        if (lane == 0) {
            out.logdet[T.o_pt] = NAN; out.off[T.o_pt] = NAN;
            out.n_low[T.o_pt] = 0; out.n_high[T.o_pt] = 0; out.sweeps[T.o_pt] = 0; out.status[T.o_pt] = 2;
        }
        return;
    }

    // 2. the sweeps
    int used = 0;
    for (int sw = 0; sw < n_sweeps; ++sw) {
        bool rotated = false;
        for (int r = 0; r < n - 1; ++r) {
            bool did = false;
            int p = 0, q = 0;
            if (lane < half) {
                const int i0 = lane == 0 ? 0 : 1 + (r + lane - 1) % (n - 1);
                const int i1 = 1 + (r + (n - 1 - lane) - 1) % (n - 1);
                p = min(i0, i1); q = max(i0, i1);
                const double apq = A[q * ls + p];
                double c = 1.0, s = 0.0;
                if (fabs(apq) > tol) {
                    const double tau = (A[q * ls + q] - A[p * ls + p]) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(fma(tau, tau, 1.0)));
                    c = 1.0 / sqrt(fma(t, t, 1.0));
                    s = t * c;
                    did = true;
                    rotated = true;
                }
                cs[2 * lane] = c; cs[2 * lane + 1] = s;
                pq[2 * lane] = p; pq[2 * lane + 1] = q;
            }
            lds_fence();
            for (int j = lane; j < n; j += 64)                 // rows: the lane's column
                for (int k = 0; k < half; ++k) {
                    const double s = cs[2 * k + 1];
                    if (s != 0.0) {
                        const double c = cs[2 * k];
                        double* ap = A + pq[2 * k] * ls + j;
                        double* aq = A + pq[2 * k + 1] * ls + j;
                        const double x = *ap, y = *aq;
                        *ap = fma(c, x, -(s * y));
                        *aq = fma(s, x, c * y);
                    }
                }
            lds_fence();
            for (int i = lane; i < n; i += 64)                 // columns and V: the lane's row
                for (int k = 0; k < half; ++k) {
                    const double s = cs[2 * k + 1];
                    if (s != 0.0) {
                        const double c = cs[2 * k];
                        const int kp = i * ls + pq[2 * k], kq = i * ls + pq[2 * k + 1];
                        const double x = A[kp], y = A[kq];
                        A[kp] = fma(c, x, -(s * y));
                        A[kq] = fma(s, x, c * y);
                        const double vx = V[kp], vy = V[kq];
                        V[kp] = fma(c, vx, -(s * vy));
                        V[kq] = fma(s, vx, c * vy);
                    }
                }
            lds_fence();
            if (did) { A[p * ls + q] = 0.0; A[q * ls + p] = 0.0; }
            lds_fence();
        }
        ++used;
        if (!__any(rotated ? 1 : 0)) break;        // (uniform) the one early exit
    }
    double off = 0.0;
    for (int i = lane; i < n; i += 64)
        for (int j = 0; j < n; ++j)
            if (j != i) off = fmax(off, fabs(A[i * ls + j]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off = fmax(off, __shfl_xor(off, o, 64));
    const bool converged = !(off > tol);

    // 3. sorted by rank counting; lam and the clamps
    for (int i = lane; i < D; i += 64) dg[i] = A[i * ls + i];
    lds_fence();
    for (int i = lane; i < D; i += 64) {
        const double e = dg[i];
        int rank = 0;
        for (int j = 0; j < D; ++j) rank += (dg[j] < e || (dg[j] == e && j < i)) ? 1 : 0;
        ord[rank] = i;
    }
    lds_fence();
    int n_low = 0, n_high = 0;
    for (int i = lane; i < D; i += 64) {
        const double e = dg[ord[i]];
        const double lam = T.kind == 0 ? e : (e > 0.0 ? 1.0 / e : INFINITY);
        n_low += lam < T.lam_lo ? 1 : 0;
        n_high += lam > T.lam_hi ? 1 : 0;
        const double lt = fmin(fmax(lam, T.lam_lo), T.lam_hi);
        w[i] = lt;
        iw[i] = 1.0 / lt;
        o_eig[i] = e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_low += __shfl_xor(n_low, o, 64);
        n_high += __shfl_xor(n_high, o, 64);
    }
    lds_fence();
    for (int e = lane; e < DD; e += 64) {
        const int i = e / D, j = e - i * D;
        o_vecs[e] = V[i * ls + ord[j]];
    }
    if (lane == 0) {
        out.off[T.o_pt] = off; out.n_low[T.o_pt] = n_low; out.n_high[T.o_pt] = n_high; out.sweeps[T.o_pt] = used;
    }
    if (!converged) {                              // (uniform) status 3
        fill(o_cov, DD, NAN, lane); fill(o_prec, DD, NAN, lane); fill(o_chol, DD, NAN, lane);
        if (lane == 0) { out.logdet[T.o_pt] = NAN; out.status[T.o_pt] = 3; }
        return;
    }

    // 4. cov and prec (cov's lower triangle into A, which is done with); ln det
    const int n_tri = D * (D + 1) / 2;
    for (int e = lane; e < n_tri; e += 64) {
        int a, b;
        tri_index(e, a, b);
        double cc = 0.0, pp = 0.0;
        for (int i = 0; i < D; ++i) {
            const int v = ord[i];
            const double va = V[a * ls + v], vb = V[b * ls + v];
            cc = fma(va * iw[i], vb, cc);
            pp = fma(va * w[i], vb, pp);
        }
        const double cv = (sc[a] * cc) * sc[b], pv = (pp / sc[a]) / sc[b];
        A[a * ls + b] = cv;
        o_cov[a * D + b] = cv; o_cov[b * D + a] = cv;
        o_prec[a * D + b] = pv; o_prec[b * D + a] = pv;
        if (a == b) sq[a] = sqrt(cv);
    }
    if (lane == 0) {
        double sl = 0.0, ss = 0.0;
        for (int i = 0; i < D; ++i) sl += log(w[i]);
        for (int d = 0; d < D; ++d) ss += log(sc[d]);
        out.logdet[T.o_pt] = sl - 2.0 * ss;
    }
    lds_fence();

    // 5. the scaled cov = L L^T; chol
    bool flat = false;
    for (int d = lane; d < D; d += 64) {
        const double v = A[d * ls + d];
        flat = flat || !(v > 0.0 && isfinite(v));
    }
    bool ok = !__any(flat ? 1 : 0);
    for (int e = lane; e < n_tri; e += 64) {
        int a, b;
        tri_index(e, a, b);
        A[a * ls + b] = A[a * ls + b] / (sq[a] * sq[b]);
    }
    lds_fence();
    const double thr = (double)D * 2.220446049250313e-16;
    for (int k = 0; k < D; ++k) {
        double piv = A[k * ls + k];
        if (!(piv > thr)) { ok = false; piv = 1.0; }
        const double l = sqrt(piv), il = 1.0 / l;
        lds_fence();
        for (int r = lane; r < D; r += 64) {
            if (r > k) A[r * ls + k] *= il;
            else if (r == k) A[k * ls + k] = l;
        }
        lds_fence();
        for (int r = lane; r < D; r += 64)
            if (r > k) {
                const double lrk = A[r * ls + k];
                for (int j = k + 1; j < D; ++j)
                    if (j <= r) A[r * ls + j] = fma(-lrk, A[j * ls + k], A[r * ls + j]);
            }
        lds_fence();
    }
    for (int e = lane; e < DD; e += 64) {
        const int i = e / D, j = e - i * D;
        o_chol[e] = ok ? (j <= i ? sq[i] * A[i * ls + j] : 0.0) : NAN;
    }
    if (lane == 0) out.status[T.o_pt] = ok ? 0 : 1;
}

}  // namespace

VAMP_METRIC_API int vamp_metric_version(void) { return VAMP_METRIC_ABI_VERSION; }

VAMP_METRIC_API const char* vamp_metric_last_error(void) { return g_err.c_str(); }

VAMP_METRIC_API int vamp_metric_plan(int max_dim, int32_t* mats_per_workgroup, int64_t* lds_bytes) {
    g_err.clear();
    if (max_dim < 1 || max_dim > kMaxDim)
        return fail("vamp_metric_plan: max_dim = " + std::to_string(max_dim) + " is outside 1 .. " + std::to_string(kMaxDim));
    const Plan p = plan(max_dim);
    if (mats_per_workgroup) *mats_per_workgroup = p.waves;
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    return 0;
}

VAMP_METRIC_API int vamp_metric_factor(int device, void* hip_stream, int n_groups, const double* const* mat, int is_device, const int64_t* ld,
                                       const int32_t* dim, const int32_t* n_mat, const double* const* scale, const int32_t* kind,
                                       const double* lam_lo, const double* lam_hi, int n_sweeps, int out_is_device, double* eig, double* vec,
                                       double* cov, double* prec, double* chol, double* logdet, int32_t* n_low, int32_t* n_high,
                                       int32_t* sweeps_used, double* off, int32_t* status) {
    g_err.clear();
    const std::string fn = "vamp_metric_factor: ";
    Layout L;
    const std::string why = check_args(fn, n_groups, mat, is_device, ld, dim, n_mat, scale, kind, lam_lo, lam_hi, n_sweeps, out_is_device, L);
    if (!why.empty()) return fail(why);
    const int G = n_groups;
    const Plan P = plan(L.max_dim);
    const long long n_tasks = L.tot_pt;
    const long long n_blocks = (n_tasks + P.waves - 1) / P.waves;
    if (n_blocks > 0x7fffffff) return fail(fn + "too many workgroups");

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (raise_lds_limit(fn, device, {{reinterpret_cast<const void*>(&k_metric), kLdsBudget}})) return -1;

    // device view of every group's matrices: staged (host input) or as given
    std::vector<const double*> dmat(mat, mat + G);
    DevBuf staging;
    if (!is_device && stage_chains(L.span, mat, st, staging, dmat)) return -1;

    std::vector<double> scales((size_t)L.tot_scale);
    std::vector<Task> tasks;
    tasks.reserve((size_t)n_tasks);
    for (int g = 0; g < G; ++g) {
        const int D = dim[g];
        for (int d = 0; d < D; ++d) scales[(size_t)L.o_scale[g] + d] = scale[g][d];
        for (int m = 0; m < n_mat[g]; ++m) {
            Task T;
            T.a = dmat[g] + (long long)m * D * ld[g];
            T.ld = ld[g];
            T.o_vec = L.o_vec[g] + (long long)m * D; T.o_mat = L.o_mat[g] + (long long)m * D * D; T.o_pt = L.o_pt[g] + m;
            T.o_scale = L.o_scale[g];
            T.lam_lo = lam_lo[g]; T.lam_hi = lam_hi[g];
            T.D = D; T.kind = kind[g];
            tasks.push_back(T);
        }
    }
    DevBuf d_tasks, d_scales, d_dbl, d_int;
    if (upload(d_tasks, tasks, st) || upload(d_scales, scales, st)) return -1;

    // one buffer of doubles: eig | logdet | off | vec | prec | cov | chol (the last two only when they stay with the library)
    const bool own = !(out_is_device && cov), own_chol = !(out_is_device && chol);
    const long long o_eig = 0, o_ld = o_eig + L.tot_vec, o_off = o_ld + L.tot_pt, o_v = o_off + L.tot_pt, o_p = o_v + L.tot_mat,
                    o_c = o_p + L.tot_mat, o_l = o_c + (own ? L.tot_mat : 0), o_end = o_l + (own_chol ? L.tot_mat : 0);
    HIP_TRY(hipMalloc(&d_dbl.p, (size_t)o_end * sizeof(double)));
    HIP_TRY(hipMalloc(&d_int.p, (size_t)L.tot_pt * 4 * sizeof(int32_t)));
    double* dd = d_dbl.as<double>();
    int32_t* di = d_int.as<int32_t>();
    Out out;
    out.eig = dd + o_eig; out.logdet = dd + o_ld; out.off = dd + o_off; out.vec = dd + o_v; out.prec = dd + o_p;
    out.cov = own ? dd + o_c : cov;
    out.chol = own_chol ? dd + o_l : chol;
    out.n_low = di; out.n_high = di + L.tot_pt; out.sweeps = di + 2 * L.tot_pt; out.status = di + 3 * L.tot_pt;

    hipLaunchKernelGGL(k_metric, dim3((unsigned)n_blocks), dim3(64 * P.waves), P.lds, st, d_tasks.as<Task>(), n_tasks, d_scales.as<double>(),
                       n_sweeps, P.slot, out);
    HIP_TRY(hipGetLastError());

    const long long sz = sizeof(double), si = sizeof(int32_t);
    if (fetch(eig, out.eig, L.tot_vec * sz, st) || fetch(logdet, out.logdet, L.tot_pt * sz, st) || fetch(off, out.off, L.tot_pt * sz, st) ||
        fetch(vec, out.vec, L.tot_mat * sz, st) || fetch(prec, out.prec, L.tot_mat * sz, st) ||
        (!out_is_device && (fetch(cov, out.cov, L.tot_mat * sz, st) || fetch(chol, out.chol, L.tot_mat * sz, st))) ||
        fetch(n_low, out.n_low, L.tot_pt * si, st) || fetch(n_high, out.n_high, L.tot_pt * si, st) ||
        fetch(sweeps_used, out.sweeps, L.tot_pt * si, st) || fetch(status, out.status, L.tot_pt * si, st))
        return -1;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
