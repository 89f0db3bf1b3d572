// chain_diag.hip -- integrated autocorrelation time, n_eff and split-R-hat of ensemble chains
// (include/vamp_diag.h, libvamp_diag.so).  Definitions: DESIGN.md "Chain diagnostics".
//
// Two launches per call:
//   k_chain_lags    one workgroup per (group, parameter, walker chunk).  The chunk's [N x Wc] tile is
//                   staged in LDS (time-major, tile[t * Wc + w]); per walker the mean, c_w(0) and the
//                   split-half means and variances; then the direct lag sums c_w(k), k = 0..N-1, register
//                   blocked R lags per lane (a ring of y_{t+k0 .. t+k0+R-1}: two LDS reads per R FMAs),
//                   normalised by c_w(0) and summed over the chunk's walkers -> rho_part[pair][chunk][k];
//                   the chunk's R-hat partials, its stuck walkers and its walkers that hold a NaN or an
//                   infinity -> stat_part[pair][chunk][6].
//   k_chain_finish  one workgroup per (group, parameter): sums the chunks, rho_bar = sum / W, prefix sum of
//                   rho_bar by wavefront shuffles until the window m >= c tau_m is found, Chan's combination
//                   of the chunks' sequence means for R-hat.  A series with a value that is not finite in any
//                   walker is answered NaN (window -1, not reliable), before "stuck" is looked at.
// Everything is fp64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/vamp_diag.h"
#include "side_call.hpp"

#define VAMP_DIAG_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace vamp::side;

constexpr int kStats = 6;          // per chunk: sequences, mean of their means, M2 of their means, sum of s^2, stuck walkers,
                                   // walkers with a value that is not finite
constexpr int kMaxWc = 64;         // walkers per chunk at most
constexpr int kSmallN = 2048;      // N <= kSmallN: R = 8 lags per lane, 256 threads; else R = 16, 512 threads
constexpr int kTileSmall = 4096;   // LDS tile budget in doubles, small-N path (32 KiB: several workgroups per CU)
constexpr int kTileLarge = VAMP_DIAG_MAX_SAMPLES + 32;   // large-N path: one walker of N = 8192 plus its padding

struct Pair {                      // one (group, parameter)
    const double* base;            // &base_g[d] (device)
    long long ld;                  // stride of t, in doubles
    long long rho_off;             // this pair's [nchunks, N] block of rho_part
    long long stat_off;            // this pair's [nchunks, kStats] block of stat_part
    int N, W, D;
    int Wc, nchunks;
    int out;                       // output slot
};

// lag sums of one chunk.  Dynamic LDS: (N + 2R) * Wc doubles; rows N .. N+2R-1 are zero so that the ring
// may run past the end of the series without a bound check.
template <int R, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_chain_lags(const Pair* __restrict__ pairs, const int2* __restrict__ tasks,
                                                      double* __restrict__ rho_part, double* __restrict__ stat_part) {
    extern __shared__ double tile[];
    __shared__ double red[5][BLOCK];
    __shared__ double w_mean[kMaxWc], w_h1[kMaxWc], w_h2[kMaxWc], w_v1[kMaxWc], w_v2[kMaxWc], w_inv[kMaxWc];
    __shared__ int w_flag[kMaxWc];                // 1: stuck (a constant series); 2: holds a NaN or an infinity

    const int2 task = tasks[blockIdx.x];
    const Pair p = pairs[task.x];
    const int N = p.N, Wc = p.Wc, tid = threadIdx.x;
    const int w0 = task.y * Wc;
    const int wn = min(Wc, p.W - w0);            // walkers of this chunk
    const int n = N / 2;                          // split-half length

    // 1. stage the tile (zero beyond the series and beyond the chunk's walkers)
    const double* src = p.base + (long long)w0 * p.D;
    const int rows = N + 2 * R;
    for (int i = tid; i < rows * Wc; i += BLOCK) {
        const int t = i / Wc, w = i - t * Wc;
        tile[i] = (t < N && w < wn) ? src[(long long)t * p.ld + (long long)w * p.D] : 0.0;
    }
    __syncthreads();

    // 2. per walker: sums of the whole series and of both halves, range (P threads per walker).  fmin / fmax skip a
    //    NaN, so a value that is not finite opens the range to (-inf, +inf): no finite series has that range
    const int P = BLOCK / Wc;
    const int w = tid % Wc, part = tid / Wc;
    const bool act = part < P && w < wn;
    {
        double s = 0.0, s1 = 0.0, s2 = 0.0, lo = INFINITY, hi = -INFINITY;
        if (act) {
            for (int t = part; t < N; t += P) {
                const double x = tile[t * Wc + w];
                s += x;
                if (t < n) s1 += x;
                if (t >= N - n) s2 += x;
                lo = fmin(lo, x);
                hi = fmax(hi, x);
                if (!(fabs(x) < INFINITY)) { lo = -INFINITY; hi = INFINITY; }
            }
        }
        red[0][tid] = s; red[1][tid] = s1; red[2][tid] = s2; red[3][tid] = lo; red[4][tid] = hi;
    }
    __syncthreads();
    if (tid < wn) {
        double s = 0.0, s1 = 0.0, s2 = 0.0, lo = INFINITY, hi = -INFINITY;
        for (int q = 0; q < P; ++q) {
            const int j = q * Wc + tid;
            s += red[0][j]; s1 += red[1][j]; s2 += red[2][j];
            lo = fmin(lo, red[3][j]); hi = fmax(hi, red[4][j]);
        }
        const bool finite = lo > -INFINITY && hi < INFINITY;
        const bool stuck = !finite || !(hi > lo); // a constant series: c_w(0) = 0 (a series that is not finite takes the
        const double x0 = tile[tid];              // same arithmetic; k_chain_finish answers its parameter NaN)
        w_flag[tid] = !finite ? 2 : stuck ? 1 : 0;
        w_mean[tid] = stuck ? x0 : s / N;
        w_h1[tid] = stuck ? x0 : s1 / n;
        w_h2[tid] = stuck ? x0 : s2 / n;
    }
    __syncthreads();

    // 3. centre in place (y = x - m_w); c_w(0) and the halves' sums of squares
    {
        double c0 = 0.0, q1 = 0.0, q2 = 0.0;
        if (act) {
            const double m = w_mean[w], h1 = w_h1[w], h2 = w_h2[w];
            for (int t = part; t < N; t += P) {
                const double x = tile[t * Wc + w];
                const double y = x - m;
                tile[t * Wc + w] = y;
                c0 = fma(y, y, c0);
                if (t < n) { const double e = x - h1; q1 = fma(e, e, q1); }
                if (t >= N - n) { const double e = x - h2; q2 = fma(e, e, q2); }
            }
        }
        red[0][tid] = c0; red[1][tid] = q1; red[2][tid] = q2;
    }
    __syncthreads();
    if (tid < wn) {
        double c0 = 0.0, q1 = 0.0, q2 = 0.0;
        for (int q = 0; q < P; ++q) {
            const int j = q * Wc + tid;
            c0 += red[0][j]; q1 += red[1][j]; q2 += red[2][j];
        }
        const bool stuck = w_flag[tid] != 0;
        w_inv[tid] = stuck ? 0.0 : 1.0 / c0;
        w_v1[tid] = stuck ? 0.0 : q1 / (n - 1);
        w_v2[tid] = stuck ? 0.0 : q2 / (n - 1);
    }
    __syncthreads();

    // 4. the chunk's R-hat partials: Welford over its 2 wn sequence means (one lane; wn <= 64)
    if (tid == 0) {
        double cnt = 0.0, mean = 0.0, m2 = 0.0, ssq = 0.0, stuck = 0.0, nonfin = 0.0;
        for (int j = 0; j < wn; ++j) {
            const double hs[2] = {w_h1[j], w_h2[j]};
            for (int h = 0; h < 2; ++h) {
                cnt += 1.0;
                const double d = hs[h] - mean;
                mean += d / cnt;
                m2 = fma(d, hs[h] - mean, m2);
            }
            ssq += w_v1[j] + w_v2[j];
            stuck += w_flag[j] & 1;
            nonfin += w_flag[j] >> 1;
        }
        double* st = stat_part + p.stat_off + (long long)task.y * kStats;
        st[0] = cnt; st[1] = mean; st[2] = m2; st[3] = ssq; st[4] = stuck; st[5] = nonfin;
    }

    // 5. lag sums: lane (s, kb) takes lags kb*R .. kb*R+R-1 of the walkers s, s+S, ... of the chunk
    const int nkb = (N + R - 1) / R;
    const int S = max(1, min(Wc, BLOCK / nkb));   // nkb <= BLOCK by the choice of R
    const int s_ = tid % S, kb = tid / S;
    double tot[R];
#pragma unroll
    for (int j = 0; j < R; ++j) tot[j] = 0.0;
    if (kb < nkb) {
        const int k0 = kb * R;
        const int T = N - k0;                      // t = 0 .. T-1 contribute to lag k0
        for (int wl = s_; wl < wn; wl += S) {
            double ring[R], acc[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                ring[j] = tile[(k0 + j) * Wc + wl];
                acc[j] = 0.0;
            }
            // ring[(u + j) % R] holds y_{t+u+k0+j}; after step u the slot of lag 0 takes y_{t+u+k0+R}
            for (int t = 0; t < T; t += R) {
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    const double yt = tile[(t + u) * Wc + wl];
#pragma unroll
                    for (int j = 0; j < R; ++j) acc[j] = fma(yt, ring[(u + j) % R], acc[j]);
                    ring[u] = tile[(t + u + k0 + R) * Wc + wl];
                }
            }
            const double iv = w_inv[wl];
#pragma unroll
            for (int j = 0; j < R; ++j) tot[j] = fma(acc[j], iv, tot[j]);
        }
    }
    __syncthreads();                               // every lane is done with the tile: reuse it as res[S][N]
    if (kb < nkb) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int k = kb * R + j;
            if (k < N) tile[s_ * N + k] = tot[j];
        }
    }
    __syncthreads();
    double* dst = rho_part + p.rho_off + (long long)task.y * N;
    for (int k = tid; k < N; k += BLOCK) {
        double v = 0.0;
        for (int q = 0; q < S; ++q) v += tile[q * N + k];
        dst[k] = v;
    }
}

__device__ inline void chan_combine(double& na, double& ma, double& m2a, double nb, double mb, double m2b) {
    if (nb == 0.0) return;
    if (na == 0.0) { na = nb; ma = mb; m2a = m2b; return; }
    const double nn = na + nb, d = mb - ma;
    ma += d * (nb / nn);
    m2a += m2b + d * d * (na * nb / nn);
    na = nn;
}

// one 256-thread workgroup per (group, parameter)
__global__ __launch_bounds__(256) void k_chain_finish(const Pair* __restrict__ pairs, const double* __restrict__ rho_part,
                                                     const double* __restrict__ stat_part, double c, double* __restrict__ tau,
                                                     double* __restrict__ n_eff, double* __restrict__ r_hat,
                                                     int32_t* __restrict__ window, uint8_t* __restrict__ reliable) {
    __shared__ double part[4][64];
    __shared__ int done;
    const Pair p = pairs[blockIdx.x];
    const int N = p.N, C = p.nchunks, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double Wd = (double)p.W;
    double carry = 0.0, tauM = NAN;
    int M = -1;
    bool found = false;
    if (tid == 0) done = 0;
    __syncthreads();
    for (int k0 = 0; k0 < N; k0 += 64) {
        const int k = k0 + lane;
        double s = 0.0;
        if (k < N)
            for (int ch = wv; ch < C; ch += 4) s += rho_part[p.rho_off + (long long)ch * N + k];
        part[wv][lane] = s;
        __syncthreads();
        if (wv == 0) {
            const double r = k < N ? (part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane]) / Wd : 0.0;
            double v = r;                          // inclusive scan over the wavefront
            for (int o = 1; o < 64; o <<= 1) {
                const double u = __shfl_up(v, o, 64);
                if (lane >= o) v += u;
            }
            const double Pk = carry + v;
            const double tau_k = 2.0 * Pk - 1.0;  // tau_m = 2 sum_{k<=m} rho_bar(k) - 1
            const unsigned long long b = __ballot(k < N && (double)k >= c * tau_k);
            if (b) {
                const int first = __ffsll((long long)b) - 1;
                tauM = __shfl(tau_k, first, 64);
                M = k0 + first;
                found = true;
                if (lane == 0) done = 1;
            } else if (k0 + 64 >= N) {             // no window up to N-1
                tauM = __shfl(tau_k, N - 1 - k0, 64);
                M = N - 1;
            }
            carry = __shfl(Pk, 63, 64);
        }
        __syncthreads();
        if (done) break;
    }
    if (wv != 0) return;
    double cnt = 0.0, mean = 0.0, m2 = 0.0, ssq = 0.0, stuck = 0.0, nonfin = 0.0;
    for (int ch = lane; ch < C; ch += 64) {
        const double* st = stat_part + p.stat_off + (long long)ch * kStats;
        chan_combine(cnt, mean, m2, st[0], st[1], st[2]);
        ssq += st[3];
        stuck += st[4];
        nonfin += st[5];
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const double cb = __shfl_down(cnt, o, 64), mb = __shfl_down(mean, o, 64), m2b = __shfl_down(m2, o, 64);
        const double sb = __shfl_down(ssq, o, 64), kb = __shfl_down(stuck, o, 64);
        const double fb = __shfl_down(nonfin, o, 64);
        if (lane + o < 64) {
            chan_combine(cnt, mean, m2, cb, mb, m2b);
            ssq += sb;
            stuck += kb;
            nonfin += fb;
        }
    }
    if (lane != 0) return;
    const double nh = (double)(N / 2), J = 2.0 * Wd;
    const double B = nh / (J - 1.0) * m2;
    const double V = ssq / J;
    double rh;
    if (V > 0.0) rh = sqrt(((nh - 1.0) / nh * V + B / nh) / V);
    else rh = B > 0.0 ? INFINITY : NAN;
    const int o = p.out;
    r_hat[o] = rh;
    if (nonfin > 0.0) {                            // a NaN or an infinity in the series of any walker: before "stuck"
        tau[o] = NAN; n_eff[o] = NAN; r_hat[o] = NAN; window[o] = -1; reliable[o] = 0;
    } else if (stuck > 0.0) {
        tau[o] = INFINITY; n_eff[o] = 0.0; window[o] = -1; reliable[o] = 0;
    } else {
        // tau_{N-1} = 0 identically, so on a chain too short to have a window tau_M can collapse to ~0 or below:
        // n_eff is NaN for tau <= 0, and reliable needs tau > 0 and N >= 50 max(tau, 1) (so N >= 50 at least)
        tau[o] = tauM;
        n_eff[o] = tauM > 0.0 ? (double)N * Wd / tauM : NAN;
        window[o] = tauM == tauM ? M : -1;
        reliable[o] = (found && tauM > 0.0 && (double)N >= 50.0 * fmax(tauM, 1.0)) ? 1 : 0;
    }
}

int walkers_per_chunk(int N) {
    const int Wc = N <= kSmallN ? kTileSmall / (N + 16) : kTileLarge / (N + 32);
    return Wc < kMaxWc ? Wc : kMaxWc;
}

}  // namespace

VAMP_DIAG_API int vamp_diag_version(void) { return VAMP_DIAG_ABI_VERSION; }

VAMP_DIAG_API const char* vamp_diag_last_error(void) { return g_err.c_str(); }

VAMP_DIAG_API int vamp_diag_chains(int device, void* hip_stream, int n_groups, const double* const* base, int is_device,
                                   const int64_t* ld, const int32_t* n_keep, const int32_t* walkers, const int32_t* ndim,
                                   double c, double* tau, double* n_eff, double* r_hat, int32_t* window, uint8_t* reliable) {
    g_err.clear();
    const std::string fn = "vamp_diag_chains: ";
    if (n_groups <= 0) return fail(fn + "n_groups must be positive");
    if (!base || !ld || !n_keep || !walkers || !ndim || !tau || !n_eff || !r_hat || !window || !reliable)
        return fail(fn + "NULL argument");
    if (!(c > 0.0) || !std::isfinite(c)) return fail(fn + "c must be a positive finite number");
    long long n_out = 0;
    for (int g = 0; g < n_groups; ++g) {
        const std::string at = fn + "group " + std::to_string(g) + ": ";
        if (!base[g]) return fail(at + "NULL base pointer");
        if (n_keep[g] <= 0 || walkers[g] <= 0 || ndim[g] <= 0) return fail(at + "n_keep, walkers and ndim must be positive");
        if (n_keep[g] > VAMP_DIAG_MAX_SAMPLES)
            return fail(at + "n_keep = " + std::to_string(n_keep[g]) + " exceeds " + std::to_string(VAMP_DIAG_MAX_SAMPLES) +
                        " (the direct lag sum is O(N^2); thin the chain)");
        if (ld[g] < (int64_t)walkers[g] * ndim[g]) return fail(at + "ld < walkers * ndim");
        n_out += ndim[g];
    }
    if (n_out > (1LL << 30)) return fail(fn + "too many outputs");

    // host-side answers first: N < 4 is NaN everywhere
    for (int g = 0, o = 0; g < n_groups; ++g)
        for (int d = 0; d < ndim[g]; ++d, ++o) {
            tau[o] = n_eff[o] = r_hat[o] = std::numeric_limits<double>::quiet_NaN();
            window[o] = -1;
            reliable[o] = 0;
        }

    DeviceRestore restore;
    if (set_device(fn, device, restore)) return -1;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);

    // device view of every group: staged (host input; N < 4 groups are answered above and not staged) or as given
    std::vector<const double*> dbase(base, base + n_groups);
    DevBuf staging;
    if (!is_device) {
        std::vector<long long> len(n_groups, 0);
        for (int g = 0; g < n_groups; ++g)
            if (n_keep[g] >= 4) len[g] = chain_span(n_keep[g], ld[g], walkers[g], ndim[g]);
        if (stage_chains(len, base, st, staging, dbase)) return -1;
    }

    // (group, parameter) pairs and their (pair, chunk) tasks, by path
    std::vector<Pair> pairs;
    std::vector<int2> tasks_small, tasks_large;
    long long rho_len = 0, stat_len = 0;
    for (int g = 0, o = 0; g < n_groups; o += ndim[g], ++g) {
        const int N = n_keep[g];
        if (N < 4) continue;
        const int Wc = walkers_per_chunk(N);
        const int nch = (walkers[g] + Wc - 1) / Wc;
        for (int d = 0; d < ndim[g]; ++d) {
            Pair p;
            p.base = dbase[g] + d;
            p.ld = ld[g];
            p.N = N; p.W = walkers[g]; p.D = ndim[g];
            p.Wc = Wc; p.nchunks = nch;
            p.out = o + d;
            p.rho_off = rho_len;
            p.stat_off = stat_len;
            rho_len += (long long)nch * N;
            stat_len += (long long)nch * kStats;
            const int pi = (int)pairs.size();
            pairs.push_back(p);
            auto& tl = N <= kSmallN ? tasks_small : tasks_large;
            for (int ch = 0; ch < nch; ++ch) tl.push_back(make_int2(pi, ch));
        }
    }
    if (pairs.empty()) return 0;
    if (tasks_small.size() > 0x7fffffff || tasks_large.size() > 0x7fffffff) return fail(fn + "too many chunks");

    DevBuf d_pairs, d_small, d_large, d_rho, d_stat, d_out, d_win, d_rel;
    const int np = (int)pairs.size();
    if (upload(d_pairs, pairs, st) || upload(d_small, tasks_small, st) || upload(d_large, tasks_large, st)) return -1;
    HIP_TRY(hipMalloc(&d_rho.p, rho_len * sizeof(double)));
    HIP_TRY(hipMalloc(&d_stat.p, stat_len * sizeof(double)));
    HIP_TRY(hipMalloc(&d_out.p, 3 * (size_t)n_out * sizeof(double)));
    HIP_TRY(hipMalloc(&d_win.p, (size_t)n_out * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&d_rel.p, (size_t)n_out));
    // slots of N < 4 groups are not written by the kernels: start from the host's NaN answers
    HIP_TRY(hipMemcpyAsync(d_out.as<double>(), tau, n_out * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_out.as<double>() + n_out, n_eff, n_out * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_out.as<double>() + 2 * n_out, r_hat, n_out * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_win.p, window, n_out * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rel.p, reliable, n_out, hipMemcpyHostToDevice, st));

    // the small path's LDS is the same for every N: (N + 16) * Wc <= kTileSmall
    if (!tasks_small.empty()) {
        hipLaunchKernelGGL((k_chain_lags<8, 256>), dim3((unsigned)tasks_small.size()), dim3(256), kTileSmall * sizeof(double), st,
                           d_pairs.as<Pair>(), d_small.as<int2>(), d_rho.as<double>(), d_stat.as<double>());
        HIP_TRY(hipGetLastError());
    }
    if (!tasks_large.empty()) {
        const size_t lds = kTileLarge * sizeof(double);   // > 64 KiB: ask for it explicitly
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chain_lags<16, 512>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_chain_lags<16, 512>), dim3((unsigned)tasks_large.size()), dim3(512), lds, st,
                           d_pairs.as<Pair>(), d_large.as<int2>(), d_rho.as<double>(), d_stat.as<double>());
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_chain_finish, dim3(np), dim3(256), 0, st, d_pairs.as<Pair>(), d_rho.as<double>(), d_stat.as<double>(), c,
                       d_out.as<double>(), d_out.as<double>() + n_out, d_out.as<double>() + 2 * n_out, d_win.as<int32_t>(),
                       d_rel.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tau, d_out.as<double>(), n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(n_eff, d_out.as<double>() + n_out, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(r_hat, d_out.as<double>() + 2 * n_out, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(window, d_win.p, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(reliable, d_rel.p, n_out, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
