// vamp_cpu.cpp -- HOST implementation of the C ABI of include/vamp_hip.h  ->  oracle/libvamp_cpu.so
//
// TEST INFRASTRUCTURE AND CPU BASELINE ONLY ("same ABI implemented by libvamp_cpu.so for the
// host baseline"; BASELINE.md Baseline B).  It lives under oracle/ on purpose: only tests/, bench.py's
// cpu_baseline leg and __graft_entry__ may load it, and only when they name it explicitly
// (vamp_amd.HipContext(lib=...)); vamp_amd itself loads libvamp_hip.so or fails.  There is no fallback.
//
// What it is for
//   * the boundary without a GPU: every entry point of the header exists here, so the ctypes layer, the VPfit
//     facade and the walker-sharded driver can be exercised in the CPU test suite;
//   * a multi-threaded C++ baseline: OpenMP over walkers, the Voigt evaluators of
//     vamp_amd/csrc/voigt_math.hpp in their host build (per pixel: J-fractions / near-axis rule; no
//     far-field interpolant, no Taylor tables).
// What it shares with libvamp_hip.so, compiled from the same headers: the argument checks, error codes and
// messages, call-order rules, region table, sampler and sharding bookkeeping of csrc/abi_state.hpp, the launch
// plan of csrc/host_plan.hpp, the draws of csrc/draws.hpp and the MAP search of csrc/map_search.hpp.  What is
// its own: the evaluation on the host (stage, lnprob_one, the OpenMP loops) and a communicator of one rank.
// It restates the same reference code as the HIP library: profiles vpfits.py:43-76, Tau2flux
// physics.py:98-105, likelihood vpfits.py:39,341, priors vpfits.py:239-252,283-297, (N,b,z) maps
// physics.py:6-27,116-134, MAP search vpfits.py:352-358 (csrc/map_search.hpp), and the stretch move of
// SURVEY Appendix B.  The independent checker of both libraries is oracle/vamp_oracle.py (scipy.wofz).
#include <omp.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../include/vamp_hip.h"
#include "../vamp_amd/csrc/abi_state.hpp"
#include "../vamp_amd/csrc/draws.hpp"
#include "../vamp_amd/csrc/host_plan.hpp"
#include "../vamp_amd/csrc/voigt_math.hpp"

namespace {

constexpr int KMAX = VAMP_MAX_COMPONENTS;
constexpr double C_LIGHT = 2.98e8;     // physics.py:3 (the reference's value)
constexpr double SIGMA0 = 0.0263;      // physics.py:4
constexpr double SQRT_LN2 = 0.83255461115769775635;
constexpr double FWHM_PER_SIGMA = 2.35482004503094938202;
const double NEG_INF = -std::numeric_limits<double>::infinity();
const double POS_INF = std::numeric_limits<double>::infinity();

using vamp::fail;
using Region = vamp::RegionDev;

struct Line { double c, s, y, amp, pole, hy; };

}  // namespace

struct vamp_ctx : vamp::AbiState {
    std::vector<double> x, f, wt;
    int threads = 1;
    // the state: X / lnp in X_own / lnp_own or in the caller's memory (vamp_sampler_bind_state: X_ext)
    bool X_ext = false;
    std::vector<double> X_own, lnp_own;
    double* X = nullptr;
    double* lnp = nullptr;
    std::vector<long long> nacc;
    std::vector<double> send, recv;        // the exchange buffers: [parts][part_slots][D+1], [parts][world*part_slots][D+1]
    bool timing = false;
    double timing_ms = 0.0;
    long long timing_launches = 0;
};

namespace {

double xexp_logp(double v) {           // vpfits.py:239-244, literally
    if (!(v >= 0.0) || !std::isfinite(v)) return NEG_INF;
    return std::log(v * std::exp(-v));
}
double uniform_logp(double v, double lo, double hi, double lp) { return (v >= lo && v <= hi) ? lp : NEG_INF; }

// parameters -> line records + log-prior (the device's stage_lines)
double stage(const Region& R, const double* t0, Line* ln) {
    double lp = 0.0;
    for (int k = 0; k < R.K; ++k) {
        const double* t = t0 + R.q * k;
        double a, c, Lw = 0.0, G = 0.0, sg = 0.0, l;
        if (R.mode == VAMP_GAUSS3) {
            a = t[0]; c = t[1]; sg = t[2];
            l = xexp_logp(a) + uniform_logp(c, R.c_lo, R.c_hi, R.lp_c) + uniform_logp(sg, 0.0, R.w_max, R.lp_w);
        } else if (R.mode == VAMP_VOIGT4) {
            a = t[0]; c = t[1]; Lw = t[2]; G = t[3];
            l = xexp_logp(a) + uniform_logp(c, R.c_lo, R.c_hi, R.lp_c) + uniform_logp(Lw, 0.0, R.w_max, R.lp_w) +
                uniform_logp(G, 0.0, R.w_max, R.lp_w);
        } else {   // NBZ3: inverse of physics.py:15,27,120,134
            const double sig = t[1] * 1.0e3 * 1.41421356237309514547 / (2.355 * (R.line * 1.0e-10));
            a = t[0] * SIGMA0 / (sig * 2.50662827463100024161);
            c = (C_LIGHT / (R.line * (1.0 + t[2]) * 1.0e-10) - R.x_origin) / R.x_scale;
            G = (sig / R.x_scale) * FWHM_PER_SIGMA;
            Lw = R.l_fixed;
            l = xexp_logp(a) + uniform_logp(c, R.c_lo, R.c_hi, R.lp_c) + uniform_logp(G, 0.0, R.w_max, R.lp_w);
        }
        Line& r = ln[k];
        r.c = c;
        if (R.mode == VAMP_GAUSS3) {
            r.s = 1.0 / sg; r.y = 0.0; r.amp = a; r.pole = 0.0; r.hy = 0.0;
        } else {
            r.s = 2.0 * SQRT_LN2 / G;
            r.y = Lw * SQRT_LN2 / G;
            r.amp = a * r.y;
            r.pole = vamp::core_pole_factor(r.y);
            r.hy = vamp::core_hy(r.y);
            if (!(r.s < POS_INF) || !(r.y < POS_INF)) l = NEG_INF;     // degenerate width: rejected, as on the device
        }
        lp += l;
    }
    if (R.sample_sd) lp += uniform_logp(t0[R.D - 1], 0.0, 1.0, 0.0);      // sd ~ U(0,1), vpfits.py:39
    return lp;
}

double loglike_from_sum(const Region& R, const double* t0, double ssum) {
    if (R.sample_sd) {
        const double sd = t0[R.D - 1], t = 1.0 / (sd * sd);
        return (double)R.P * 0.5 * std::log(t / (2.0 * vamp::PI)) - 0.5 * t * ssum;      // vpfits.py:39,341
    }
    return -0.5 * ssum + R.norm_const;                                                   // vpfits.py:118
}

// log-posterior of one parameter vector; chi receives the (weighted) sum of squared residuals
double lnprob_one(const vamp_ctx* c, const Region& R, const double* t0, double* chi_out) {
    Line ln[KMAX];
    const double lp = stage(R, t0, ln);
    if (!(lp > NEG_INF) || lp != lp) {
        if (chi_out) *chi_out = std::numeric_limits<double>::quiet_NaN();
        return NEG_INF;
    }
    const double *x = c->x.data() + R.pix_off, *f = c->f.data() + R.pix_off, *wt = c->wt.data() + R.pix_off;
    double chi = 0.0;
    if (c->f32) {       // fp32 pixel arithmetic, Humlicek W4, chi^2 accumulated in fp64 (BASELINE.json config 5)
        for (int i = 0; i < R.P; ++i) {
            float tau = 0.0f;
            const float xi = (float)x[i];
            for (int k = 0; k < R.K; ++k) {
                const float u = std::fabs(xi - (float)ln[k].c) * (float)ln[k].s;
                if (R.mode == VAMP_GAUSS3) tau += (float)ln[k].amp * std::exp(-0.5f * (u * u));
                else tau += (float)(ln[k].amp * vamp::SQRT_PI) * vamp::humlicek_w4_re(std::fmin(u, vamp::W4_XMAX), (float)ln[k].y);
            }
            const float m = std::exp(-tau), r = ((float)f[i] - m) * (float)wt[i];
            chi += (double)r * (double)r;
        }
    } else {
        double dtab[KMAX][vamp::DTAB_N];
        if (R.mode != VAMP_GAUSS3)
            for (int k = 0; k < R.K; ++k)
                for (int n = 0; n < vamp::DTAB_N; ++n) dtab[k][n] = vamp::core_dtab_entry(n, ln[k].y);
        for (int i = 0; i < R.P; ++i) {
            double tau = 0.0;
            for (int k = 0; k < R.K; ++k) {
                if (R.mode == VAMP_GAUSS3) {
                    const double u = (x[i] - ln[k].c) * ln[k].s;
                    tau += ln[k].amp * std::exp(-0.5 * (u * u));
                } else {
                    tau += ln[k].amp * vamp::voigt_Hs(std::fabs(x[i] - ln[k].c) * ln[k].s, ln[k].y, dtab[k], ln[k].pole, ln[k].hy);
                }
            }
            const double r = (f[i] - std::exp(-tau)) * wt[i];
            chi += r * r;
        }
    }
    if (chi_out) *chi_out = chi;
    double v = lp + loglike_from_sum(R, t0, chi);
    if (v != v) v = NEG_INF;                 // NaN -> -inf (emcee convention)
    return v;
}

void lnprob_block(const vamp_ctx* c, int region, long long W, const double* theta, double* out, double* chi) {
    const Region& R = c->regions_h[region];
#pragma omp parallel for schedule(dynamic, 4) num_threads(c->threads)
    for (long long w = 0; w < W; ++w) {
        double ch;
        out[w] = lnprob_one(c, R, theta + w * R.D, &ch);
        if (chi) chi[w] = ch;
    }
}

int lnprob_all_impl(const vamp_ctx* c, long long W, const double* theta, double* out, double* chi) {
    for (int r = 0; r < c->n_regions; ++r)
        lnprob_block(c, r, W, theta + W * c->regions_h[r].d_before, out + (long long)r * W, chi ? chi + (long long)r * W : nullptr);
    return 0;
}

// one mover: propose, evaluate, accept; pk (may be null) receives the row it ends with
void move_one(vamp_ctx* c, const Region& R, long long ws, long long wc, double z, double logu, double* pk) {
    double q[4 * KMAX + 1];
    double* Xs = c->X + R.theta_off + ws * R.D;
    const double* Xc = c->X + R.theta_off + wc * R.D;
    for (int d = 0; d < R.D; ++d) q[d] = Xc[d] - (Xc[d] - Xs[d]) * z;        // q = c - (c - s) z
    const double lnp_q = lnprob_one(c, R, q, nullptr);
    const long long wg = R.walker_off + ws;
    const double lnp_s = c->lnp[wg];
    const double diff = (double)(R.D - 1) * std::log(z) + lnp_q - lnp_s;
    const bool accept = logu < diff;                                        // false for NaN
    if (pk) {
        for (int d = 0; d < R.D; ++d) pk[d] = accept ? q[d] : Xs[d];
        pk[R.D] = accept ? lnp_q : lnp_s;
    }
    if (accept) {
        for (int d = 0; d < R.D; ++d) Xs[d] = q[d];
        c->lnp[wg] = lnp_q;
        c->nacc[wg] += 1;
    }
}

// piece `part` of this ctx's share of one half-step.  Movers write only their own rows and read only
// rows of the frozen colour, so the loop is parallel and the update is in place.
void half_step_part(vamp_ctx* c, int half, int part) {
    const auto t0 = std::chrono::steady_clock::now();
    const long long halfW = c->W / 2;
    long long lo, hi;
    if (c->n_regions == 1) {
        lo = c->slot_begin + part * c->part_stride;
        hi = c->shard_parts > 1 ? lo + c->part_slots : c->slot_end;
    } else {
        lo = 0;
        hi = c->total_walkers / 2;
    }
    const unsigned step = (unsigned)c->step;
    double* pack = c->exchange ? c->send.data() + part * vamp::part_doubles(c, false) : nullptr;
    if (pack) {
        c->part_step[part] = step;
        c->part_half[part] = half;
    }
#pragma omp parallel for schedule(dynamic, 4) num_threads(c->threads)
    for (long long slot = lo; slot < hi; ++slot) {
        const int region = (int)(slot / halfW);
        const Region& R = c->regions_h[region];
        const vamp::MoveDraw d = vamp::draw_move(*c, step, half, region, slot - (long long)region * halfW);
        move_one(c, R, d.ws, d.wc, d.z, d.logu, pack ? pack + (slot - lo) * (R.D + 1) : nullptr);
    }
    if (c->timing) {
        c->timing_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        c->timing_launches += 1;
    }
}

// rows of piece `part` gathered from all ranks -> walker rows (the device's k_scatter_rows)
void scatter_part(vamp_ctx* c, int part, const double* rows) {
    const Region& R = c->regions_h[0];
    const long long n_rows = (long long)c->shard_world * c->part_slots, own_lo = (long long)c->shard_rank * c->part_slots;
    for (long long i = 0; i < n_rows; ++i) {
        if (i >= own_lo && i < own_lo + c->part_slots) continue;
        const long long slot = (long long)part * c->part_stride + i;
        const unsigned hb = (unsigned)(c->split_block >> 1), chunk = (unsigned)(slot / hb), pos = (unsigned)(slot % hb);
        const long long ws = (long long)chunk * c->split_block + vamp::split_perm(c->seed, c->part_step[part], chunk, (unsigned)R.rng_id,
                                                                                   pos + (c->part_half[part] ? hb : 0u), (unsigned)c->split_block);
        const double* src = rows + i * (R.D + 1);
        std::memcpy(c->X + R.theta_off + ws * R.D, src, R.D * sizeof(double));
        c->lnp[R.walker_off + ws] = src[R.D];
    }
}

void half_step_all(vamp_ctx* c, int half) {
    for (int p = 0; p < c->shard_parts; ++p) {
        half_step_part(c, half, p);
        if (c->comm && c->exchange) {       // a communicator of one rank: the gather is a self-copy
            const size_t n = vamp::part_doubles(c, false);
            std::memcpy(c->recv.data() + (size_t)p * n, c->send.data() + (size_t)p * n, n * sizeof(double));
            scatter_part(c, p, c->recv.data() + (size_t)p * n);
        }
    }
}

void free_sampler(vamp_ctx* c) {
    c->X_own.clear(); c->lnp_own.clear(); c->nacc.clear(); c->send.clear(); c->recv.clear();
    if (!c->X_ext) { c->X = nullptr; c->lnp = nullptr; }
    c->exchange = false;
    c->sampler_ready = false;
}

// the exchange buffers of the shard (vamp_sampler_set_shard_parts, or vamp_comm_init_rank after it)
void alloc_exchange_buffers(vamp_ctx* c) {
    c->send.assign(vamp::exchange_send_doubles(c), 0.0);
    c->recv.assign(vamp::exchange_recv_doubles(c), 0.0);
    vamp::exchange_parts(c);
    c->exchange = true;
}

}  // namespace

extern "C" {

int vamp_version(void) { return VAMP_ABI_VERSION; }
const char* vamp_last_error(void) { return vamp::last_error().c_str(); }
int vamp_device_count(int* n) {
    if (int rc = vamp::check_device_count(n)) return rc;
    *n = 1;                       // the host
    return VAMP_OK;
}

int vamp_ctx_create(vamp_ctx** out, int device, int dtype, int wofz_kind) {
    if (int rc = vamp::check_ctx_create(out, dtype, wofz_kind)) return rc;
    if (int rc = vamp::check_device(device, 1)) return rc;
    vamp_ctx* c = nullptr;
    if (int rc = vamp::new_ctx(&c, dtype)) return rc;
    c->threads = omp_get_max_threads();
    if (const char* e = getenv("VAMP_CPU_THREADS")) c->threads = std::max(1, atoi(e));
    *out = c;
    return VAMP_OK;
}
int vamp_ctx_destroy(vamp_ctx* c) { delete c; return VAMP_OK; }
int vamp_ctx_set_stream(vamp_ctx* c, void*) { return vamp::need_ctx(c, "vamp_ctx_set_stream"); }
int vamp_ctx_set_stream_default(vamp_ctx* c) { return vamp::need_ctx(c, "vamp_ctx_set_stream_default"); }
int vamp_ctx_synchronize(vamp_ctx* c) { return vamp::need_ctx(c, "vamp_ctx_synchronize"); }
// the switches choose between device execution forms with identical results: nothing to switch on the host
int vamp_ctx_set_option(vamp_ctx* c, const char* name, int64_t) { return vamp::check_option(c, name); }
// a launch shape: nothing to launch on the host, but the class plan follows it
int vamp_ctx_set_packing(vamp_ctx* c, int lanes) { return vamp::set_packing(c, lanes); }

int vamp_set_regions(vamp_ctx* c, int n_regions, const int64_t* pix_off, const double* x, const double* flux,
                     const double* noise, const int32_t* n_comp, int mode, int sample_sd, int include_norm,
                     const double* bounds, const double* nbz) {
    if (int rc = vamp::check_set_regions(c, n_regions, pix_off, x, flux, noise, n_comp, mode, nbz)) return rc;
    free_sampler(c);
    // (the launch plan of the HIP library is computed here too: nothing is launched on the host, but the product's own plan
    // arithmetic runs -- under the sanitizers in the _asan build -- and vamp_region_class answers)
    if (int rc = vamp::build_regions(c, n_regions, pix_off, x, noise, n_comp, mode, sample_sd, include_norm, bounds, nbz, true)) return rc;
    const long long N = pix_off[n_regions];
    c->x.assign(x, x + N);
    c->f.assign(flux, flux + N);
    c->wt = vamp::pixel_weights(N, noise, sample_sd);
    c->n_regions = n_regions;
    return VAMP_OK;
}

int vamp_region_class(vamp_ctx* c, int region, int* kind, int* n_classes) { return vamp::region_class(c, region, kind, n_classes); }
int vamp_set_region_ids(vamp_ctx* c, const int32_t* ids) { return vamp::set_region_ids(c, ids); }
int vamp_region_ndim(vamp_ctx* c, int region, int* ndim) { return vamp::region_ndim(c, region, ndim); }

int vamp_lnprob(vamp_ctx* c, int region, int64_t W, const double* theta, double* lnprob, double* chi2) {
    if (int rc = vamp::check_lnprob(c, region, W, theta, lnprob)) return rc;
    lnprob_block(c, region, W, theta, lnprob, chi2);
    return VAMP_OK;
}

int vamp_lnprob_all(vamp_ctx* c, int64_t W, const double* theta, double* lnprob, double* chi2) {
    if (int rc = vamp::check_lnprob_all(c, W, theta, lnprob)) return rc;
    return lnprob_all_impl(c, W, theta, lnprob, chi2);
}

int vamp_map_all(vamp_ctx* c, const double* theta0, const uint8_t* active, int64_t maxiter, int64_t maxfun, double xtol,
                 double ftol, double* theta_best, double* lnprob_best, double* chi2_best, int64_t* iterations) {
    if (int rc = vamp::check_map_all(c, theta0, maxiter, maxfun, xtol, ftol, theta_best, lnprob_best)) return rc;
    int rc = vamp::map_search_host(c, theta0, active, maxiter, maxfun, xtol, ftol, theta_best, iterations,
                                   [&](int W, const double* th, double* lp) { return lnprob_all_impl(c, W, th, lp, nullptr); });
    if (rc) return rc;
    return lnprob_all_impl(c, 1, theta_best, lnprob_best, chi2_best);
}

int vamp_model(vamp_ctx* c, int region, const double* theta1, double* tau_comp, double* flux_model) {
    if (int rc = vamp::check_model(c, "vamp_model", region, theta1)) return rc;
    const Region& R = c->regions_h[region];
    Line ln[KMAX];
    (void)stage(R, theta1, ln);
    double dtab[vamp::DTAB_N];
    std::vector<double> tau(R.P, 0.0);
    for (int k = 0; k < R.K; ++k) {
        if (R.mode != VAMP_GAUSS3)
            for (int n = 0; n < vamp::DTAB_N; ++n) dtab[n] = vamp::core_dtab_entry(n, ln[k].y);
        for (int i = 0; i < R.P; ++i) {
            const double xi = c->x[R.pix_off + i];
            double tk;
            if (R.mode == VAMP_GAUSS3) {
                const double u = (xi - ln[k].c) * ln[k].s;
                tk = ln[k].amp * std::exp(-0.5 * (u * u));
            } else {
                tk = ln[k].amp * vamp::voigt_Hs(std::fabs(xi - ln[k].c) * ln[k].s, ln[k].y, dtab, ln[k].pole, ln[k].hy);
            }
            if (tau_comp) tau_comp[(long long)k * R.P + i] = tk;
            tau[i] += tk;
        }
    }
    if (flux_model)
        for (int i = 0; i < R.P; ++i) flux_model[i] = std::exp(-tau[i]);
    return VAMP_OK;
}

int vamp_model_all(vamp_ctx* c, const double* theta, double* tau_comp, double* flux_model) {
    if (int rc = vamp::check_model_all(c, theta)) return rc;
    for (int r = 0; r < c->n_regions; ++r) {
        const Region& R = c->regions_h[r];
        int rc = vamp_model(c, r, theta + R.d_before, tau_comp ? tau_comp + R.tau_off : nullptr,
                            flux_model ? flux_model + R.pix_off : nullptr);
        if (rc) return rc;
    }
    return VAMP_OK;
}

int vamp_line_records(vamp_ctx* c, int region, const double* theta1, double* rec, double* lnprior) {
    if (int rc = vamp::check_model(c, "vamp_line_records", region, theta1 && rec && lnprior)) return rc;
    const Region& R = c->regions_h[region];
    Line ln[KMAX];
    *lnprior = stage(R, theta1, ln);
    for (int k = 0; k < R.K; ++k) {
        rec[5 * k + 0] = ln[k].c; rec[5 * k + 1] = ln[k].s; rec[5 * k + 2] = ln[k].y;
        rec[5 * k + 3] = (R.mode == VAMP_GAUSS3) ? ln[k].amp : ln[k].amp * vamp::SQRT_PI;
        rec[5 * k + 4] = ln[k].pole;
    }
    return VAMP_OK;
}

int vamp_wofz_re(vamp_ctx* c, int64_t n, const double* x, const double* y, double* re_w) {
    if (int rc = vamp::check_wofz(c, n, x, y, re_w)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        if (c->f32) {
            re_w[i] = (double)vamp::humlicek_w4_re(std::fmin(std::fabs((float)x[i]), vamp::W4_XMAX), (float)y[i]);
        } else {
            double dtab[vamp::DTAB_N];
            for (int k = 0; k < vamp::DTAB_N; ++k) dtab[k] = vamp::core_dtab_entry(k, y[i]);
            re_w[i] = vamp::voigt_H(std::fabs(x[i]), y[i], dtab, vamp::core_pole_factor(y[i]), vamp::core_hy(y[i]));
        }
    }
    return VAMP_OK;
}

// ---- sampler ---------------------------------------------------------------------------------
int vamp_sampler_bind_state(vamp_ctx* c, void* X_dev, void* lnp_dev) {
    if (int rc = vamp::check_bind_state(c, X_dev, lnp_dev)) return rc;
    free_sampler(c);
    c->X = (double*)X_dev;       // host memory here
    c->lnp = (double*)lnp_dev;
    c->X_ext = true;
    return VAMP_OK;
}

int vamp_sampler_init(vamp_ctx* c, int64_t W, const double* theta0, uint64_t seed, double a, int32_t split_block) {
    if (int rc = vamp::check_sampler_init(c, W, theta0, a, split_block)) return rc;
    const bool ext = c->X_ext && c->X;
    if (!ext) free_sampler(c);
    vamp::init_sampler(c, W, seed, a, split_block);
    if (!ext) {
        c->X_ext = false;
        c->X_own.resize(c->total_theta);
        c->lnp_own.resize(c->total_walkers);
        c->X = c->X_own.data();
        c->lnp = c->lnp_own.data();
    }
    c->nacc.assign(c->total_walkers, 0);
    c->send.clear(); c->recv.clear();
    std::memcpy(c->X, theta0, c->total_theta * sizeof(double));
    lnprob_all_impl(c, W, c->X, c->lnp, nullptr);
    c->sampler_ready = true;
    return VAMP_OK;
}

int vamp_sampler_set_shard_parts(vamp_ctx* c, int rank, int world, int parts, int64_t* own_begin, int64_t* own_end) {
    if (int rc = vamp::set_shard_parts(c, rank, world, parts, own_begin, own_end)) return rc;
    c->send.clear(); c->recv.clear();
    if (vamp::needs_exchange(c)) alloc_exchange_buffers(c);
    return VAMP_OK;
}
int vamp_sampler_set_shard(vamp_ctx* c, int rank, int world, int64_t* own_begin, int64_t* own_end) {
    return vamp_sampler_set_shard_parts(c, rank, world, 1, own_begin, own_end);
}

int vamp_sampler_state_ptrs(vamp_ctx* c, void** X_dev, void** lnp_dev, int64_t* total_theta, int64_t* total_walkers) {
    if (int rc = vamp::need_sampler(c, "vamp_sampler_state_ptrs")) return rc;
    if (X_dev) *X_dev = c->X;
    if (lnp_dev) *lnp_dev = c->lnp;
    if (total_theta) *total_theta = c->total_theta;
    if (total_walkers) *total_walkers = c->total_walkers;
    return VAMP_OK;
}

int vamp_sampler_half_step(vamp_ctx* c, int half) {
    if (int rc = vamp::check_half_step(c, half)) return rc;
    half_step_all(c, half);
    if (half == 1) c->step += 1;
    return VAMP_OK;
}

int vamp_sampler_half_step_part(vamp_ctx* c, int half, int part) {
    if (int rc = vamp::check_half_step_part(c, half, part)) return rc;
    half_step_part(c, half, part);
    if (half == 1 && part == c->shard_parts - 1) c->step += 1;
    return VAMP_OK;
}

int vamp_sampler_half_step_ext(vamp_ctx* c, int region, int64_t n, const int32_t* active_idx, const int32_t* partner_idx,
                               const double* zz, const double* logu) {
    if (int rc = vamp::check_half_step_ext(c, region, n, active_idx, partner_idx, zz, logu)) return rc;
    const Region& R = c->regions_h[region];
#pragma omp parallel for schedule(dynamic, 4) num_threads(c->threads)
    for (int64_t i = 0; i < n; ++i) move_one(c, R, active_idx[i], partner_idx[i], zz[i], logu[i], nullptr);
    return VAMP_OK;
}

int vamp_sampler_run_dev(vamp_ctx* c, int64_t n_steps, int thin, double* chain_dev, double* lnprob_chain_dev, double* seconds) {
    if (int rc = vamp::check_run(c, true, n_steps, thin)) return rc;
    const long long n_keep = n_steps / thin;
    const auto t0 = std::chrono::steady_clock::now();
    long long kept = 0;
    for (long long it = 0; it < n_steps; ++it) {
        half_step_all(c, 0);
        half_step_all(c, 1);
        c->step += 1;
        if ((it + 1) % thin == 0 && kept < n_keep) {
            if (chain_dev) std::memcpy(chain_dev + kept * c->total_theta, c->X, c->total_theta * sizeof(double));
            if (lnprob_chain_dev) std::memcpy(lnprob_chain_dev + kept * c->total_walkers, c->lnp, c->total_walkers * sizeof(double));
            ++kept;
        }
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return VAMP_OK;
}

int vamp_sampler_run(vamp_ctx* c, int64_t n_steps, int thin, double* chain, double* lnprob_chain, int64_t* n_accept, double* seconds) {
    if (int rc = vamp::check_run(c, false, n_steps, thin)) return rc;
    int rc = vamp_sampler_run_dev(c, n_steps, thin, chain, lnprob_chain, seconds);      // "device" memory is host memory here
    if (rc) return rc;
    if (n_accept) std::memcpy(n_accept, c->nacc.data(), c->total_walkers * sizeof(long long));
    return VAMP_OK;
}

int vamp_sampler_get_state(vamp_ctx* c, double* theta, double* lnprob, int64_t* n_accept, int64_t* step) {
    if (int rc = vamp::need_sampler(c, "vamp_sampler_get_state")) return rc;
    if (theta) std::memcpy(theta, c->X, c->total_theta * sizeof(double));
    if (lnprob) std::memcpy(lnprob, c->lnp, c->total_walkers * sizeof(double));
    if (n_accept) std::memcpy(n_accept, c->nacc.data(), c->total_walkers * sizeof(long long));
    if (step) *step = c->step;
    return VAMP_OK;
}

int vamp_sampler_set_state(vamp_ctx* c, const double* theta, const double* lnprob, int64_t step) {
    if (int rc = vamp::check_set_state(c, theta, lnprob, step)) return rc;
    std::memcpy(c->X, theta, c->total_theta * sizeof(double));
    std::memcpy(c->lnp, lnprob, c->total_walkers * sizeof(double));
    c->step = step;
    return VAMP_OK;
}

// ---- multi-device entry points: the host build has no RCCL; a communicator of ONE rank is accepted
//      so that the single-rank rehearsal of the exchange runs through the same call sequence ----
int vamp_comm_unique_id(char* id) {
    if (int rc = vamp::check_unique_id(id)) return rc;
    std::memset(id, 0, VAMP_COMM_ID_BYTES);
    std::memcpy(id, "vamp-cpu", 8);
    return VAMP_OK;
}
int vamp_comm_init_rank(vamp_ctx* c, const char* id, int rank, int world) {
    if (int rc = vamp::check_comm_init_rank(c, id, rank, world)) return rc;
    if (world != 1) return fail(VAMP_ERR_COMM, "vamp_comm_init_rank: the host build has no RCCL (exchange through vamp_sampler_pack_get / scatter_put)");
    if (vamp::join_comm(c, rank, world) && !c->exchange) alloc_exchange_buffers(c);
    return VAMP_OK;
}
int vamp_comm_library(char* path, int64_t capacity) {
    // the host build has no RCCL: its one-rank "communicator" is this library itself
    if (int rc = vamp::check_comm_library(path, capacity)) return rc;
    Dl_info info;
    const char* name = (dladdr(reinterpret_cast<void*>(&vamp_comm_library), &info) && info.dli_fname) ? info.dli_fname : "";
    std::snprintf(path, (size_t)capacity, "%s", name);
    return VAMP_OK;
}
int vamp_comm_destroy(vamp_ctx* c) {
    if (int rc = vamp::need_ctx(c, "vamp_comm_destroy")) return rc;
    vamp::leave_comm(c);
    return VAMP_OK;
}
int vamp_comm_info(vamp_ctx* c, int* rank, int* world, int* queried) {
    if (int rc = vamp::check_comm_info(c)) return rc;
    if (rank) *rank = c->comm_rank;
    if (world) *world = c->comm_world;
    if (queried) *queried = 0;
    return VAMP_OK;
}

int vamp_sampler_pack_get(vamp_ctx* c, int part, double* rows) {
    if (int rc = vamp::check_exchange_rows(c, false, part, rows)) return rc;
    const size_t n = vamp::part_doubles(c, false);
    std::memcpy(rows, c->send.data() + (size_t)part * n, n * sizeof(double));
    return VAMP_OK;
}
int vamp_sampler_scatter_put(vamp_ctx* c, int part, const double* rows_all) {
    if (int rc = vamp::check_exchange_rows(c, true, part, rows_all)) return rc;
    scatter_part(c, part, rows_all);
    return VAMP_OK;
}

// ---- test hooks (not part of the ABI: no vamp_ prefix): the launch-plan arithmetic of csrc/host_plan.hpp that no host
//      entry point reaches, so that tests/test_cpu_boundary.py -- and its sanitizer run -- can drive it -----------------
long long vampdbg_xcd_map(long long b, long long n_regions, long long bpr) { return vamp::plan::xcd_map(b, n_regions, bpr); }
void vampdbg_packed_grid(long long n_regions, long long half_w, int subs, int waves_per_block, long long* out3) {
    const vamp::plan::PackedGrid g = vamp::plan::plan_packed_grid(n_regions, half_w, subs, waves_per_block);
    out3[0] = g.wpr; out3[1] = g.grid; out3[2] = g.bpr;
}
int vampdbg_resident_class_ok(int kind, long long half_w, int compute_waves, int walkers_per_wave, int automatic) {
    return vamp::plan::resident_class_ok(kind, half_w, compute_waves, walkers_per_wave, automatic != 0) ? 1 : 0;
}

int vamp_exchange_timing(vamp_ctx* c, double* total_ms, int64_t* exchanges) {
    if (int rc = vamp::need_ctx(c, "vamp_exchange_timing")) return rc;
    if (total_ms) *total_ms = 0.0;          // the host build has no in-library exchange
    if (exchanges) *exchanges = 0;
    return VAMP_OK;
}

int vamp_kernel_timing(vamp_ctx* c, int enable, double* total_ms, int64_t* launches) {
    if (int rc = vamp::need_ctx(c, "vamp_kernel_timing")) return rc;
    if (total_ms) *total_ms = c->timing_ms;
    if (launches) *launches = c->timing_launches;
    c->timing_ms = 0.0;
    c->timing_launches = 0;
    c->timing = enable != 0;
    return VAMP_OK;
}

}  // extern "C"
