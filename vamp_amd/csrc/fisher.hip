// fisher.hip -- gradient of the log-posterior, Gauss-Newton information matrix and its inverse at given parameter
// vectors, from the analytic Jacobian of the model flux (include/vamp_fisher.h, libvamp_fisher.so).  Definitions:
// DESIGN.md section 15.
//
// One launch of k_fisher, one workgroup of 256 threads per (group, point):
//   1. the point's lines become line records once (lane_group.hpp's line_record; a bad point ends here with NaN
//      outputs and status 2), and every Voigt line gets its near-axis table, in LDS
//   2. the pixels in tiles of 64: wavefront s of the four owns the lines s, s + 4, ... of the tile's 64 pixels -- one
//      pixel per lane, so a wavefront works on one line at a time -- and writes their d tau / d theta (voigt_grad.hpp)
//      into the pixel's row of the LDS tile and its share of tau to the pixel's slot; after a barrier the four shares
//      are added in slot order, f = exp(-tau), and each thread turns what it wrote into a_pd = J_pd / sigma_p (J itself
//      goes to jac when it is asked for)
//   3. the D (D + 1) / 2 entries of the information are dealt over the 256 threads, entry e to thread e mod 256; each
//      adds its entries over the tile's pixels in pixel order, tile after tile, in registers; thread d adds grad_d and
//      the last thread chi^2 the same way.  No sum depends on anything but the point.
//   4. the prior's terms, the free sd's row; the scaled matrix C_ij = I_ij / (sqrt I_ii sqrt I_jj) into the tile's LDS
//   5. the first wavefront factorises C = L L^T (a lane per row), inverts L (a lane per column: X = L^-1 goes into the
//      upper triangle, its diagonal into an array of its own); every loop runs to D.  A pivot that is not above
//      D 2^-52 makes the point's status 1.
//   6. all threads: S = X^T X, cov_ij = S_ij / (sqrt I_ii sqrt I_jj), sigma, ln det I = sum ln I_ii + 2 sum ln L_ii.
// Everything is fp64; results leave the kernel by ordinary vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vamp_fisher.h"
#include "lane_group.hpp"
#include "side_call.hpp"
#include "voigt_grad.hpp"
#include "voigt_math.hpp"

#define VAMP_FISHER_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace vamp::side;
using vamp::lds_fence;

constexpr int kBlock = 256;
constexpr int kTile = 64;                  // pixels of a tile: one per lane
constexpr int kSlots = kBlock / kTile;     // wavefronts that share a tile's lines
constexpr int kRec = 6;                    // doubles of a line record
constexpr int kMaxK = VAMP_FISHER_MAX_COMPONENTS;
constexpr int kMaxD = VAMP_FISHER_MAX_DIM;
constexpr int kStride = kMaxD + 1;         // row stride of the tile and of the matrix
constexpr int kEnt = (kMaxD * (kMaxD + 1) / 2 + kBlock - 1) / kBlock;     // entries of a triangle per thread: 9
static_assert(kMaxD == 4 * kMaxK + 1, "D = q K + sample_sd");
static_assert(kMaxD * kStride >= kTile * kStride, "the matrix reuses the tile");

struct Group {
    const double* x;               // device copies of the region
    const double* flux;
    const double* noise;           // NULL: free sd
    const double* theta;           // the group's points (device)
    long long ld;                  // doubles between two points
    long long o_vec, o_mat, o_pt, o_jac;      // where the group's first point starts in the outputs
    int P, K, q, sd, D;
};

struct Out {
    double *grad, *info, *cov, *sigma, *logdet, *chi2, *jac;      // jac may be NULL
    int32_t* status;
};

// entry e of a lower triangle stored row by row: e = i (i + 1) / 2 + j, j <= i
__device__ __forceinline__ void tri_index(int e, int& i, int& j) {
    i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > e) --i;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    j = e - i * (i + 1) / 2;
}

__global__ __launch_bounds__(kBlock) void k_fisher(const Group* __restrict__ groups, const int2* __restrict__ tasks, int with_prior,
                                                   Out out) {
    __shared__ double s_a[kMaxD * kStride];            // the tile's rows a_pd; then C, L and X
    __shared__ double s_tk[kTile * (kSlots + 1)];      // the slots' shares of tau
    __shared__ double s_rs[kTile];                     // r_p / sigma_p
    __shared__ double s_rec[kMaxK * kRec];
    __shared__ double s_dtab[kMaxK * vamp::DTAB_N];
    __shared__ double s_th[kMaxD + 1], s_dg[kMaxD + 1], s_sq[kMaxD + 1], s_xd[kMaxD + 1];
    __shared__ double s_chi2, s_logdet;
    __shared__ int s_ok;

    const int2 task = tasks[blockIdx.x];
    const Group G = groups[task.x];
    const int tid = threadIdx.x;
    const int P = G.P, K = G.K, q = G.q, D = G.D, Dl = q * K;
    const bool voigt = q == 4;
    const long long pt = task.y;
    double* o_grad = out.grad + G.o_vec + pt * D;
    double* o_sigma = out.sigma + G.o_vec + pt * D;
    double* o_info = out.info + G.o_mat + pt * D * D;
    double* o_cov = out.cov + G.o_mat + pt * D * D;
    double* o_jac = out.jac ? out.jac + G.o_jac + pt * P * D : nullptr;
    const long long o_pt = G.o_pt + pt;

    // 1. the point and its line records
    if (tid < D) s_th[tid] = G.theta[pt * G.ld + tid];
    __syncthreads();
    bool bad = false;
    if (tid < K) bad = vamp::line_record(voigt, s_th + q * tid, s_rec + tid * kRec);
    const double sd = G.sd ? s_th[D - 1] : 1.0;
    if (G.sd && tid == 0) bad = bad || !(isfinite(sd) && sd > 0.0);
    if (__syncthreads_or(bad ? 1 : 0)) {
        for (int d = tid; d < D; d += kBlock) { o_grad[d] = NAN; o_sigma[d] = NAN; }
        for (int e = tid; e < D * D; e += kBlock) { o_info[e] = NAN; o_cov[e] = NAN; }
        if (o_jac) for (long long e = tid; e < (long long)P * D; e += kBlock) o_jac[e] = NAN;
        if (tid == 0) { out.logdet[o_pt] = NAN; out.chi2[o_pt] = NAN; out.status[o_pt] = 2; }
        return;
    }
    if (voigt) vamp::fill_dtab<kRec>(s_dtab, s_rec, K, tid, kBlock);

    // the thread's entries of the lines' block of the information
    const int n_ent = Dl * (Dl + 1) / 2;
    int ei[kEnt], ej[kEnt];
    double acc[kEnt];
#pragma unroll
    for (int m = 0; m < kEnt; ++m) {
        int i = 0, j = 0;
        if (tid + m * kBlock < n_ent) tri_index(tid + m * kBlock, i, j);
        ei[m] = i;
        ej[m] = j;
        acc[m] = 0.0;
    }
    double gacc = 0.0, cacc = 0.0;
    __syncthreads();

    // 2., 3. the pixels, a tile at a time
    const int pix = tid & (kTile - 1), slot = tid / kTile;
    for (int p0 = 0; p0 < P; p0 += kTile) {
        const int np = min(kTile, P - p0);
        double* row = s_a + pix * kStride;
        if (pix < np) {
            const double xi = G.x[p0 + pix];
            double tsum = 0.0;
            for (int k = slot; k < K; k += kSlots) {
                const double* r = s_rec + k * kRec;
                const double* th = s_th + q * k;
                double* a = row + q * k;
                if (voigt) {
                    const double u = (xi - r[0]) * r[1];
                    const vamp::VoigtGrad g = vamp::voigt_grad(u, r[2], s_dtab + k * vamp::DTAB_N, r[4], r[5]);
                    tsum += r[3] * g.Ks;
                    a[0] = r[2] * g.Ks;
                    a[1] = -(r[3] * vamp::SQRT_PI) * r[1] * g.Ku;
                    a[2] = (th[0] * vamp::SQRT_PI) * (0.5 * r[1]) * g.TL;
                    a[3] = -((r[3] * vamp::SQRT_PI) / th[3]) * g.TG;
                } else {
                    const double u = (xi - r[0]) * r[1];
                    const double e = exp(-0.5 * (u * u));
                    const double ae = th[0] * e;
                    tsum += ae;
                    a[0] = e;
                    a[1] = ae * u * r[1];
                    a[2] = ae * (u * u) * r[1];
                }
            }
            s_tk[pix * (kSlots + 1) + slot] = tsum;
        }
        __syncthreads();
        if (pix < np) {
            const double* tk = s_tk + pix * (kSlots + 1);
            const double tau = ((tk[0] + tk[1]) + tk[2]) + tk[3];      // slot order
            const double f = exp(-tau);
            const double is = 1.0 / (G.noise ? G.noise[p0 + pix] : sd);
            if (slot == 0) {
                s_rs[pix] = (G.flux[p0 + pix] - f) * is;
                if (o_jac && G.sd) o_jac[(long long)(p0 + pix) * D + Dl] = 0.0;
            }
            for (int k = slot; k < K; k += kSlots)
                for (int j = 0; j < q; ++j) {
                    const double v = -f * row[q * k + j];
                    if (o_jac) o_jac[(long long)(p0 + pix) * D + q * k + j] = v;
                    row[q * k + j] = v * is;
                }
        }
        __syncthreads();
        for (int p = 0; p < np; ++p) {                                  // pixel order
            const double* a = s_a + p * kStride;
#pragma unroll
            for (int m = 0; m < kEnt; ++m)
                if (tid + m * kBlock < n_ent) acc[m] = fma(a[ei[m]], a[ej[m]], acc[m]);
            const double rs = s_rs[p];
            if (tid < Dl) gacc = fma(a[tid], rs, gacc);
            if (tid == kBlock - 1) cacc = fma(rs, rs, cacc);
        }
        __syncthreads();
    }

    // 4. chi^2, the prior's terms, the free sd; the diagonal
    if (tid == kBlock - 1) { s_chi2 = cacc; out.chi2[o_pt] = cacc; }
    if (tid < Dl) {
        if (with_prior && tid % q == 0) gacc += 1.0 / s_th[tid] - 1.0;
        o_grad[tid] = gacc;
    }
#pragma unroll
    for (int m = 0; m < kEnt; ++m)
        if (tid + m * kBlock < n_ent) {
            const int i = ei[m], j = ej[m];
            if (with_prior && i == j && i % q == 0) acc[m] += 1.0 / (s_th[i] * s_th[i]);
            o_info[i * D + j] = acc[m];
            o_info[j * D + i] = acc[m];
            if (i == j) s_dg[i] = acc[m];
        }
    __syncthreads();
    if (G.sd) {
        if (tid < Dl) { o_info[Dl * D + tid] = 0.0; o_info[tid * D + Dl] = 0.0; }
        if (tid == 0) {
            const double v = 2.0 * (double)P / (sd * sd);
            o_info[Dl * D + Dl] = v;
            s_dg[Dl] = v;
            o_grad[Dl] = s_chi2 / sd - (double)P / sd;
        }
    }
    __syncthreads();
    bool flat = false;
    if (tid < D) {
        flat = !(s_dg[tid] > 0.0 && isfinite(s_dg[tid]));
        s_sq[tid] = sqrt(s_dg[tid]);
    }
    const bool not_pd = __syncthreads_or(flat ? 1 : 0) != 0;
    // the scaled matrix, lower triangle (the tile is done with)
#pragma unroll
    for (int m = 0; m < kEnt; ++m)
        if (tid + m * kBlock < n_ent) s_a[ei[m] * kStride + ej[m]] = acc[m] / (s_sq[ei[m]] * s_sq[ej[m]]);
    if (G.sd) {
        if (tid < Dl) s_a[Dl * kStride + tid] = 0.0;
        if (tid == 0) s_a[Dl * kStride + Dl] = s_dg[Dl] / (s_sq[Dl] * s_sq[Dl]);
    }
    __syncthreads();

    // 5. the first wavefront: C = L L^T, X = L^-1
    if (tid < 64) {
        const int lane = tid;
        bool ok = !not_pd;
        const double thr = (double)D * 2.220446049250313e-16;
        for (int k = 0; k < D; ++k) {
            double piv = s_a[k * kStride + k];
            if (!(piv > thr)) { ok = false; piv = 1.0; }
            const double l = sqrt(piv), il = 1.0 / l;
            lds_fence();
            for (int r = lane; r < D; r += 64) {
                if (r > k) s_a[r * kStride + k] *= il;
                else if (r == k) s_a[k * kStride + k] = l;
            }
            lds_fence();
            for (int r = lane; r < D; r += 64)
                if (r > k) {
                    const double lrk = s_a[r * kStride + k];
                    for (int j = k + 1; j < D; ++j)
                        if (j <= r) s_a[r * kStride + j] = fma(-lrk, s_a[j * kStride + k], s_a[r * kStride + j]);
                }
            lds_fence();
        }
        // column j of X by forward substitution; X_ij (i > j) goes to row j of the upper triangle
        for (int j = lane; j < D; j += 64) {
            const double xjj = 1.0 / s_a[j * kStride + j];
            s_xd[j] = xjj;
            for (int i = 0; i < D; ++i)
                if (i > j) {
                    double sum = 0.0;
                    for (int k = 0; k < D; ++k)
                        if (k >= j && k < i) sum = fma(s_a[i * kStride + k], k == j ? xjj : s_a[j * kStride + k], sum);
                    s_a[j * kStride + i] = -sum / s_a[i * kStride + i];
                }
        }
        if (lane == 0) {
            double ld = 0.0;
            for (int i = 0; i < D; ++i) ld += log(s_dg[i]) + 2.0 * log(s_a[i * kStride + i]);
            s_logdet = ld;
            s_ok = ok ? 1 : 0;
        }
    }
    __syncthreads();

    // 6. cov = X^T X unscaled, sigma, logdet, status
    const bool ok = s_ok != 0;
    const int n_all = D * (D + 1) / 2;
#pragma unroll
    for (int m = 0; m < kEnt; ++m) {
        const int e = tid + m * kBlock;
        if (e < n_all) {
            int i, j;
            tri_index(e, i, j);
            double v = NAN;
            if (ok) {
                double sum = 0.0;
                for (int k = i; k < D; ++k) {
                    const double xi = k == i ? s_xd[i] : s_a[i * kStride + k];
                    const double xj = k == j ? s_xd[j] : s_a[j * kStride + k];
                    sum = fma(xi, xj, sum);
                }
                v = sum / (s_sq[i] * s_sq[j]);
            }
            o_cov[i * D + j] = v;
            o_cov[j * D + i] = v;
            if (i == j) o_sigma[i] = sqrt(v);
        }
    }
    if (tid == 0) {
        out.logdet[o_pt] = ok ? s_logdet : NAN;
        out.status[o_pt] = ok ? 0 : 1;
    }
}

bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace

VAMP_FISHER_API int vamp_fisher_version(void) { return VAMP_FISHER_ABI_VERSION; }

VAMP_FISHER_API const char* vamp_fisher_last_error(void) { return g_err.c_str(); }

VAMP_FISHER_API int vamp_fisher_points(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                                       const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                                       const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                                       const int32_t* n_points, int with_prior, double* grad, double* info, double* cov,
                                       double* sigma, double* logdet, double* chi2, int32_t* status, double* jac) {
    g_err.clear();
    const std::string fn = "vamp_fisher_points: ";
    if (n_groups <= 0) return fail(fn + "n_groups must be positive");
    if (!x || !flux || !noise || !n_pix || !n_comp || !mode || !sample_sd || !base || !ld || !n_points) return fail(fn + "NULL argument");
    long long tot_pix = 0, tot_vec = 0, tot_mat = 0, tot_pt = 0, tot_jac = 0;
    std::vector<int> Dg(n_groups);
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (n_pix[g] < 1) return fail(at + "n_pix must be at least 1");
        if (n_comp[g] < 1 || n_comp[g] > VAMP_FISHER_MAX_COMPONENTS)
            return fail(at + "n_comp = " + std::to_string(n_comp[g]) + " is outside 1 .. " + std::to_string(VAMP_FISHER_MAX_COMPONENTS));
        if (mode[g] == 2) return fail(at + "mode 2 (NBZ3) is not supported");
        if (mode[g] != 0 && mode[g] != 1) return fail(at + "unknown mode " + std::to_string(mode[g]));
        if (sample_sd[g] != 0 && sample_sd[g] != 1) return fail(at + "sample_sd must be 0 or 1");
        if (!x[g] || !flux[g] || !base[g]) return fail(at + "NULL array");
        if ((noise[g] == nullptr) != (sample_sd[g] == 1)) return fail(at + "noise must be NULL exactly when sample_sd is set");
        if (!all_finite(x[g], n_pix[g]) || !all_finite(flux[g], n_pix[g])) return fail(at + "x and flux must be finite");
        if (noise[g]) {
            if (!all_finite(noise[g], n_pix[g])) return fail(at + "noise must be finite");
            for (int p = 0; p < n_pix[g]; ++p)
                if (!(noise[g][p] > 0.0)) return fail(at + "noise must be positive");
        }
        const int D = (mode[g] == 1 ? 4 : 3) * n_comp[g] + sample_sd[g];
        Dg[g] = D;
        if (n_points[g] < 1) return fail(at + "n_points must be at least 1");
        if (ld[g] < (n_points[g] > 1 ? D : 0))
            return fail(at + "ld = " + std::to_string((long long)ld[g]) + " is below the " + std::to_string(D) + " parameters of a point");
        tot_pix += n_pix[g];
        tot_vec += (long long)n_points[g] * D;
        tot_mat += (long long)n_points[g] * D * D;
        tot_pt += n_points[g];
        tot_jac += (long long)n_points[g] * n_pix[g] * D;
        if (tot_mat > VAMP_FISHER_MAX_MATRIX_DOUBLES || tot_pix > (1LL << 30))
            return fail(fn + "more than " + std::to_string(VAMP_FISHER_MAX_MATRIX_DOUBLES) + " matrix entries (sum of n_points D^2): split the call");
        if (jac && tot_jac > VAMP_FISHER_MAX_MATRIX_DOUBLES)
            return fail(fn + "more than " + std::to_string(VAMP_FISHER_MAX_MATRIX_DOUBLES) + " Jacobian entries (sum of n_points P D): split the call");
    }
    if (!jac) tot_jac = 0;

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    // device view of every group's points: staged (host input) or as given
    std::vector<const double*> dbase(base, base + n_groups);
    DevBuf staging;
    if (!is_device) {
        std::vector<long long> len(n_groups);
        for (int g = 0; g < n_groups; ++g) len[g] = (long long)(n_points[g] - 1) * ld[g] + Dg[g];
        if (stage_chains(len, base, st, staging, dbase)) return -1;
    }

    // one buffer of doubles: x | flux | noise | grad | sigma | info | cov | logdet | chi2 | jac
    const long long o_x = 0, o_f = o_x + tot_pix, o_n = o_f + tot_pix, o_g = o_n + tot_pix, o_s = o_g + tot_vec, o_i = o_s + tot_vec,
                    o_c = o_i + tot_mat, o_l = o_c + tot_mat, o_q = o_l + tot_pt, o_j = o_q + tot_pt, o_end = o_j + tot_jac;
    DevBuf d_main, d_status;
    HIP_TRY(hipMalloc(&d_main.p, (size_t)o_end * sizeof(double)));
    HIP_TRY(hipMalloc(&d_status.p, (size_t)tot_pt * sizeof(int32_t)));
    double* dm = d_main.as<double>();

    std::vector<Group> groups(n_groups);
    std::vector<int2> tasks;
    tasks.reserve((size_t)tot_pt);
    long long pix = 0, vec = 0, mat = 0, pts = 0, jo = 0;
    for (int g = 0; g < n_groups; ++g) {
        const size_t nb = (size_t)n_pix[g] * sizeof(double);
        HIP_TRY(hipMemcpyAsync(dm + o_x + pix, x[g], nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dm + o_f + pix, flux[g], nb, hipMemcpyHostToDevice, st));
        if (noise[g]) HIP_TRY(hipMemcpyAsync(dm + o_n + pix, noise[g], nb, hipMemcpyHostToDevice, st));
        Group& G = groups[g];
        G.x = dm + o_x + pix; G.flux = dm + o_f + pix; G.noise = noise[g] ? dm + o_n + pix : nullptr;
        G.theta = dbase[g]; G.ld = ld[g];
        G.o_vec = vec; G.o_mat = mat; G.o_pt = pts; G.o_jac = jo;
        G.P = n_pix[g]; G.K = n_comp[g]; G.q = mode[g] == 1 ? 4 : 3; G.sd = sample_sd[g]; G.D = Dg[g];
        for (int i = 0; i < n_points[g]; ++i) tasks.push_back(make_int2(g, i));
        pix += n_pix[g];
        vec += (long long)n_points[g] * Dg[g];
        mat += (long long)n_points[g] * Dg[g] * Dg[g];
        pts += n_points[g];
        if (jac) jo += (long long)n_points[g] * n_pix[g] * Dg[g];
    }
    if (tasks.size() > 0x7fffffff) return fail(fn + "too many workgroups");

    DevBuf d_groups, d_tasks;
    if (upload(d_groups, groups, st) || upload(d_tasks, tasks, st)) return -1;
    Out out;
    out.grad = dm + o_g; out.sigma = dm + o_s; out.info = dm + o_i; out.cov = dm + o_c; out.logdet = dm + o_l; out.chi2 = dm + o_q;
    out.jac = jac ? dm + o_j : nullptr;
    out.status = d_status.as<int32_t>();
    hipLaunchKernelGGL(k_fisher, dim3((unsigned)tasks.size()), dim3(kBlock), 0, st, d_groups.as<Group>(), d_tasks.as<int2>(),
                       with_prior ? 1 : 0, out);
    HIP_TRY(hipGetLastError());

    const long long sz = sizeof(double);
    if (fetch(grad, dm + o_g, tot_vec * sz, st) || fetch(sigma, dm + o_s, tot_vec * sz, st) || fetch(info, dm + o_i, tot_mat * sz, st) ||
        fetch(cov, dm + o_c, tot_mat * sz, st) || fetch(logdet, dm + o_l, tot_pt * sz, st) || fetch(chi2, dm + o_q, tot_pt * sz, st) ||
        fetch(jac, dm + o_j, tot_jac * sz, st) || fetch(status, d_status.p, tot_pt * (long long)sizeof(int32_t), st))
        return -1;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
