// abi_state.hpp -- what the two implementations of include/vamp_hip.h share, whatever runs their arithmetic: the error
// reporting, the region table (struct RegionDev), the state every vamp_ctx carries (struct AbiState: regions, class plan,
// sampler scalars, shard and part bookkeeping, communicator), the argument and call-order checks of the entry points and
// the bookkeeping behind them.  No HIP in here: like host_plan.hpp it is compiled into libvamp_hip.so
// (csrc/vamp_hip.hip: device memory, launches, streams, RCCL) and into oracle/libvamp_cpu.so (oracle/vamp_cpu.cpp: the
// host evaluation), whose AddressSanitizer + UndefinedBehaviorSanitizer build runs it under tests/test_sanitizers.py.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vamp_hip.h"
#include "host_plan.hpp"
#include "map_search.hpp"

namespace vamp {

// ---- errors: every entry point returns a VAMP_ERR_* code and leaves its message for vamp_last_error ----------------
inline std::string& last_error() {
    thread_local std::string msg;
    return msg;
}
inline int fail(int code, const std::string& msg) {
    last_error() = msg;
    return code;
}

// ---- one region (one posterior), as the kernels read it ----------------------------------------------------------
struct RegionDev {
    long long pix_off;     // into x / flux / wt
    long long theta_off;   // doubles: start of this region's [W, D] block in the sampler state
    long long walker_off;  // first global walker id of this region in the sampler state
    long long d_before;    // sum of D over the preceding regions (vamp_lnprob_all: block r starts at W * d_before)
    long long tau_off;     // sum of K * P over the preceding regions (vamp_model_all: this region's tau_comp block)
    long long sim_off;     // sum of (D + 1) * D over the preceding regions (k_map_search: this region's simplex)
    int P, K, mode, D;     // D = q*K (+1 if sample_sd)
    int sample_sd, q, rng_id, pad1;   // rng_id: the region's identity in the draw keys (default: its index)
    double c_lo, c_hi;     // centroid prior (vpfits.py:250,293)
    double w_max;          // sigma_max (GAUSS3, vpfits.py:320) or fwhm_max (vpfits.py:326)
    double lp_c, lp_w;     // -log(c_hi - c_lo), -log(w_max): uniform log-densities
    double l_fixed, line, x_origin, x_scale;   // NBZ3
    double norm_const;     // -1/2 sum log(2 pi sigma^2) or 0
    double tile_span;      // plan::Limits::tile * (largest pixel spacing of the region)
};

// ---- the state of a context that does not depend on where the arithmetic runs (each vamp_ctx derives from it) -------
struct AbiState {
    int dtype = VAMP_F64;
    bool f32 = false;
    // regions (n_regions == 0: none set)
    int n_regions = 0;
    int mode = VAMP_VOIGT4;
    int packing = 0;                   // vamp_ctx_set_packing: 0 = auto, 16 / 64 / 65 / 256 lanes per walker
    std::vector<RegionDev> regions_h;
    plan::ClassPlan plan;              // the launch classes of the regions (vamp_region_class)
    plan::ClassPlan plan_small;        // ... of small ensembles: the short-region classes merged
    // sampler
    bool sampler_ready = false;
    long long W = 0, total_theta = 0, total_walkers = 0;
    int split_block = 0;
    double a = 2.0;
    unsigned long long seed = 0;
    long long step = 0;
    // this context's share of the active slots: part 0 (the whole share when shard_parts == 1)
    long long slot_begin = 0, slot_end = 0;
    int shard_rank = 0, shard_world = 1, shard_parts = 1;
    long long part_slots = 0, part_stride = 0;   // slots per part; distance between this rank's parts
    // walker-sharded runs: active-colour exchange (pack -> all-gather -> scatter)
    bool exchange = false;             // the exchange buffers of the shard exist
    std::vector<unsigned> part_step;   // (step, half) of the last half-step of every part
    std::vector<int> part_half;
    bool comm = false;                 // a communicator (vamp_comm_init_rank) ...
    int comm_rank = 0, comm_world = 1; // ... and its rank and size
};

// region r's identity in the draw keys (draws.hpp)
inline int region_rng_id(const AbiState& c, int r) { return c.regions_h[r].rng_id; }

// ---- checks shared by many entry points: `fn` names the entry point in the message --------------------------------
inline int bad_arg(const char* fn, const std::string& what) { return fail(VAMP_ERR_ARG, std::string(fn) + ": " + what); }
inline int bad_state(const char* fn, const std::string& what) { return fail(VAMP_ERR_STATE, std::string(fn) + ": " + what); }
inline int need_ctx(const AbiState* c, const char* fn) { return c ? VAMP_OK : bad_arg(fn, "ctx is NULL"); }
inline int need_regions(const AbiState* c, const char* fn) {
    return c->n_regions ? VAMP_OK : bad_state(fn, "call vamp_set_regions first");
}
inline int need_region(const AbiState* c, int region, const char* fn) {
    return (region >= 0 && region < c->n_regions) ? VAMP_OK : bad_arg(fn, "no such region");
}
inline int need_sampler(const AbiState* c, const char* fn) {
    if (!c) return bad_arg(fn, "ctx is NULL");
    return c->sampler_ready ? VAMP_OK : bad_state(fn, "call vamp_sampler_init first");
}
constexpr int MAX_REGIONS_PER_LAUNCH = 65535;      // one grid row per region
inline int need_launchable(const AbiState* c, const char* fn) {
    return c->n_regions <= MAX_REGIONS_PER_LAUNCH ? VAMP_OK : bad_arg(fn, "at most 65535 regions per launch");
}

// ---- contexts -------------------------------------------------------------------------------------------------------
inline int check_device_count(const int* n) { return n ? VAMP_OK : bad_arg("vamp_device_count", "n is NULL"); }
inline int check_ctx_create(void* out, int dtype, int wofz_kind) {
    if (!out) return bad_arg("vamp_ctx_create", "out is NULL");
    if (!((dtype == VAMP_F64 && wofz_kind == VAMP_WOFZ_ACCURATE) || (dtype == VAMP_F32 && wofz_kind == VAMP_WOFZ_HUMLICEK_W4)))
        return bad_arg("vamp_ctx_create", "supported pairs are (F64, ACCURATE) and (F32, HUMLICEK_W4)");
    return VAMP_OK;
}
inline int check_device(int device, int n_devices) {
    return (device >= 0 && device < n_devices) ? VAMP_OK : bad_arg("vamp_ctx_create", "no such device");
}
// a new context of the given precision (Ctx: the library's vamp_ctx)
template <class Ctx>
int new_ctx(Ctx** out, int dtype) {
    *out = new (std::nothrow) Ctx();
    if (!*out) return fail(VAMP_ERR_NOMEM, "vamp_ctx_create: host allocation failed");
    (*out)->dtype = dtype;
    (*out)->f32 = dtype == VAMP_F32;
    return VAMP_OK;
}
inline int set_packing(AbiState* c, int lanes) {
    if (int rc = need_ctx(c, "vamp_ctx_set_packing")) return rc;
    if (lanes != 0 && lanes != 16 && lanes != 64 && lanes != 65 && lanes != 256)
        return bad_arg("vamp_ctx_set_packing", "lanes_per_walker must be 0 (auto), 16, 64, 65 (64 + per-walker tables) or 256");
    c->packing = lanes;
    return VAMP_OK;
}
inline int check_option(const AbiState* c, const char* name) {
    if (!c || !name) return bad_arg("vamp_ctx_set_option", "NULL argument");
    const std::string key(name);
    if (key != "map_device" && key != "resident" && key != "class_streams")
        return bad_arg("vamp_ctx_set_option", "unknown option '" + key + "' (map_device, resident, class_streams)");
    return VAMP_OK;
}

// ---- regions --------------------------------------------------------------------------------------------------------
inline int check_set_regions(const AbiState* c, int n_regions, const int64_t* pix_off, const double* x, const double* flux,
                             const double* noise, const int32_t* n_comp, int mode, const double* nbz) {
    const char* fn = "vamp_set_regions";
    if (!c || n_regions <= 0 || !pix_off || !x || !flux || !noise || !n_comp) return bad_arg(fn, "NULL argument or n_regions <= 0");
    if (mode != VAMP_GAUSS3 && mode != VAMP_VOIGT4 && mode != VAMP_NBZ3) return bad_arg(fn, "bad mode");
    if (mode == VAMP_NBZ3 && !nbz) return bad_arg(fn, "VAMP_NBZ3 needs nbz");
    if (pix_off[0] != 0) return bad_arg(fn, "pix_off[0] must be 0");
    if (n_regions > MAX_REGIONS_PER_LAUNCH) return bad_arg(fn, "at most 65535 regions per context (one grid row per region)");
    return VAMP_OK;
}

// The region table of vamp_set_regions (its arguments checked by check_set_regions) into c->regions_h, and the launch
// classes of the regions into c->plan / c->plan_small (tables_f32: fp32 contexts have single-precision Taylor rows for
// their blends).  Sets the mode, leaves n_regions at 0: the library sets it once it holds the regions' data.
inline int build_regions(AbiState* c, int n_regions, const int64_t* pix_off, const double* x, const double* noise,
                         const int32_t* n_comp, int mode, int sample_sd, int include_norm, const double* bounds, const double* nbz,
                         bool tables_f32) {
    const char* fn = "vamp_set_regions";
    const plan::Limits lim;
    c->n_regions = 0;
    c->mode = mode;
    const int q = (mode == VAMP_VOIGT4) ? 4 : 3;
    std::vector<RegionDev>& R = c->regions_h;
    R.assign(n_regions, RegionDev());
    for (int r = 0; r < n_regions; ++r) {
        const long long P = pix_off[r + 1] - pix_off[r];
        if (P < 2 || P > 0x7fffffff) return bad_arg(fn, "a region needs >= 2 pixels");
        if (n_comp[r] < 1 || n_comp[r] > VAMP_MAX_COMPONENTS) return bad_arg(fn, "n_comp out of range (1..32)");
        RegionDev& d = R[r];
        std::memset(&d, 0, sizeof(d));
        d.pix_off = pix_off[r];
        d.P = (int)P;
        d.K = n_comp[r];
        d.mode = mode;
        d.q = q;
        d.sample_sd = sample_sd ? 1 : 0;
        d.rng_id = r;
        d.D = q * d.K + d.sample_sd;
        d.d_before = r ? R[r - 1].d_before + R[r - 1].D : 0;
        d.tau_off = r ? R[r - 1].tau_off + (long long)R[r - 1].K * R[r - 1].P : 0;
        d.sim_off = r ? R[r - 1].sim_off + (long long)(R[r - 1].D + 1) * R[r - 1].D : 0;
        const double* xr = x + pix_off[r];
        if (bounds) {
            d.c_lo = bounds[4 * r + 0];
            d.c_hi = bounds[4 * r + 1];
            d.w_max = (mode == VAMP_GAUSS3) ? bounds[4 * r + 2] : bounds[4 * r + 3];
        } else {
            d.c_lo = std::min(xr[0], xr[P - 1]);             // vpfits.py:250 (the reference's grid ascends)
            d.c_hi = std::max(xr[0], xr[P - 1]);
            const double sigma_max = (d.c_hi - d.c_lo) / 2.0;                         // vpfits.py:320
            d.w_max = (mode == VAMP_GAUSS3) ? sigma_max : sigma_max * 2 * std::sqrt(2 * std::log(2.0));   // :326
        }
        if (!(d.c_hi > d.c_lo) || !(d.w_max > 0)) return bad_arg(fn, "empty prior range");
        d.lp_c = -std::log(d.c_hi - d.c_lo);
        d.lp_w = -std::log(d.w_max);
        if (mode == VAMP_NBZ3) {
            d.l_fixed = nbz[4 * r + 0];
            d.line = nbz[4 * r + 1];
            d.x_origin = nbz[4 * r + 2];
            d.x_scale = nbz[4 * r + 3];
        }
        double nc = 0.0;
        if (include_norm && !sample_sd) {
            for (long long i = 0; i < P; ++i) {
                const double s = noise[pix_off[r] + i];
                nc += std::log(2.0 * M_PI * s * s);
            }
            nc *= -0.5;
        }
        d.norm_const = nc;
        // the tile code takes a tile's first and last pixel as its extent: the grid of a region must be
        // strictly monotonic (either direction; the reference sorts to ascending frequency,
        // vpspectrum.py:274-277) and finite
        double dxmax = 0.0;
        const bool up = xr[1] > xr[0];
        for (long long i = 1; i < P; ++i) {
            const double dx = xr[i] - xr[i - 1];
            if (!std::isfinite(dx) || dx == 0.0 || (dx > 0.0) != up)
                return bad_arg(fn, "x must be finite and strictly monotonic within a region");
            dxmax = std::max(dxmax, std::fabs(dx));
        }
        d.tile_span = lim.tile * dxmax;
    }
    // launch classes (csrc/host_plan.hpp, plan_classes): both partitions
    std::vector<plan::RegionShape> shp(n_regions);
    for (int r = 0; r < n_regions; ++r) shp[r] = plan::RegionShape{R[r].P, R[r].K};
    const std::string err = plan::plan_classes(shp, c->packing, mode == VAMP_GAUSS3, c->f32, tables_f32, c->plan, lim);
    if (!err.empty()) return bad_arg(fn, err);
    (void)plan::plan_classes(shp, c->packing, mode == VAMP_GAUSS3, c->f32, tables_f32, c->plan_small, lim, true);
    return VAMP_OK;
}
// 1 / sigma per pixel, or 1 where the noise is sampled (sample_sd)
inline std::vector<double> pixel_weights(long long n_pix, const double* noise, int sample_sd) {
    std::vector<double> wt(n_pix);
    for (long long i = 0; i < n_pix; ++i) wt[i] = sample_sd ? 1.0 : 1.0 / noise[i];
    return wt;
}

inline int set_region_ids(AbiState* c, const int32_t* ids) {
    if (!c || !ids) return bad_arg("vamp_set_region_ids", "NULL argument");
    if (int rc = need_regions(c, "vamp_set_region_ids")) return rc;
    for (int r = 0; r < c->n_regions; ++r)
        if (ids[r] < 0) return bad_arg("vamp_set_region_ids", "ids must be >= 0");
    for (int r = 0; r < c->n_regions; ++r) c->regions_h[r].rng_id = ids[r];
    return VAMP_OK;
}
inline int region_class(const AbiState* c, int region, int* kind, int* n_classes) {
    if (int rc = need_ctx(c, "vamp_region_class")) return rc;
    if (int rc = need_region(c, region, "vamp_region_class")) return rc;
    if (kind) *kind = c->plan.kind[c->plan.class_of[region]];
    if (n_classes) *n_classes = (int)c->plan.kind.size();
    return VAMP_OK;
}
inline int region_ndim(const AbiState* c, int region, int* ndim) {
    if (!c || !ndim) return bad_arg("vamp_region_ndim", "NULL argument");
    if (int rc = need_region(c, region, "vamp_region_ndim")) return rc;
    *ndim = c->regions_h[region].D;
    return VAMP_OK;
}

// ---- evaluations ----------------------------------------------------------------------------------------------------
inline int check_lnprob(const AbiState* c, int region, long long W, const double* theta, const double* lnprob) {
    if (!c || !theta || !lnprob) return bad_arg("vamp_lnprob", "NULL argument");
    if (int rc = need_regions(c, "vamp_lnprob")) return rc;
    if (int rc = need_region(c, region, "vamp_lnprob")) return rc;
    return W > 0 ? VAMP_OK : bad_arg("vamp_lnprob", "W must be positive");
}
inline int check_lnprob_all(const AbiState* c, long long W, const double* theta, const double* lnprob) {
    if (!c || !theta || !lnprob) return bad_arg("vamp_lnprob_all", "NULL argument");
    if (int rc = need_regions(c, "vamp_lnprob_all")) return rc;
    if (W <= 0) return bad_arg("vamp_lnprob_all", "W must be positive");
    return need_launchable(c, "vamp_lnprob_all");
}
inline int check_map_all(const AbiState* c, const double* theta0, long long maxiter, long long maxfun, double xtol, double ftol,
                         const double* theta_best, const double* lnprob_best) {
    if (!c || !theta0 || !theta_best || !lnprob_best) return bad_arg("vamp_map_all", "NULL argument");
    if (int rc = need_regions(c, "vamp_map_all")) return rc;
    if (int rc = need_launchable(c, "vamp_map_all")) return rc;
    if (maxiter < 0 || maxfun < 0 || !(xtol >= 0.0) || !(ftol >= 0.0)) return bad_arg("vamp_map_all", "bad limits");
    return VAMP_OK;
}
// the host-driven MAP search of every region (csrc/map_search.hpp); lnprob_all(W, theta, lnprob) evaluates W points of
// every region
template <class F>
int map_search_host(const AbiState* c, const double* theta0, const uint8_t* active, long long maxiter, long long maxfun, double xtol,
                    double ftol, double* theta_best, int64_t* iterations, F&& lnprob_all) {
    std::vector<int> dims(c->n_regions);
    std::vector<long long> offs(c->n_regions);
    for (int r = 0; r < c->n_regions; ++r) {
        dims[r] = c->regions_h[r].D;
        offs[r] = c->regions_h[r].d_before;
    }
    return nelder_mead_all(c->n_regions, dims.data(), offs.data(), theta0, active, maxiter, maxfun, xtol, ftol, theta_best, iterations,
                           lnprob_all);
}
// vamp_model and vamp_line_records (args: the pointers that must not be NULL are not), and vamp_model_all
inline int check_model(const AbiState* c, const char* fn, int region, bool args) {
    if (!c || !args) return bad_arg(fn, "NULL argument");
    if (int rc = need_regions(c, fn)) return rc;
    return need_region(c, region, fn);
}
inline int check_model_all(const AbiState* c, const double* theta) {
    if (!c || !theta) return bad_arg("vamp_model_all", "NULL argument");
    return need_regions(c, "vamp_model_all");
}
inline int check_wofz(const AbiState* c, long long n, const double* x, const double* y, const double* re_w) {
    return (!c || !x || !y || !re_w || n <= 0) ? bad_arg("vamp_wofz_re", "bad argument") : VAMP_OK;
}

// ---- sampler --------------------------------------------------------------------------------------------------------
inline int check_bind_state(const AbiState* c, const void* X, const void* lnp) {
    return (!c || !X || !lnp) ? bad_arg("vamp_sampler_bind_state", "NULL argument") : VAMP_OK;
}
inline int check_sampler_init(const AbiState* c, long long W, const double* theta0, double a, int split_block) {
    const char* fn = "vamp_sampler_init";
    if (!c || !theta0) return bad_arg(fn, "NULL argument");
    if (int rc = need_regions(c, fn)) return rc;
    if (W < 2 || (W & 1)) return bad_arg(fn, "W must be even and >= 2");
    if (split_block < 2 || (split_block & 1) || W % split_block) return bad_arg(fn, "split_block must be even and divide W");
    if (!(a > 1.0)) return bad_arg(fn, "a must be > 1");
    return VAMP_OK;
}
// vamp_sampler_init's bookkeeping: the regions' blocks in the state (theta_off, walker_off), the sampler scalars, one
// shard of the whole ensemble; the library then fills the state and sets sampler_ready
inline void init_sampler(AbiState* c, long long W, unsigned long long seed, double a, int split_block) {
    long long tt = 0;
    for (int r = 0; r < c->n_regions; ++r) {
        c->regions_h[r].theta_off = tt;
        c->regions_h[r].walker_off = (long long)r * W;
        tt += W * c->regions_h[r].D;
    }
    c->sampler_ready = false;
    c->W = W;
    c->total_theta = tt;
    c->total_walkers = (long long)c->n_regions * W;
    c->split_block = split_block;
    c->a = a;
    c->seed = seed;
    c->step = 0;
    c->shard_rank = 0;
    c->shard_world = 1;
    c->shard_parts = 1;
    c->part_slots = c->part_stride = 0;
    c->slot_begin = 0;
    c->slot_end = c->total_walkers / 2;
    c->exchange = false;
}

// vamp_sampler_set_shard_parts: the checks, the shard's bookkeeping (csrc/host_plan.hpp: the ensemble is cut into
// `parts` equal row ranges and each of those into `world` shards) and the walker rows it owns.  The exchange buffers
// are the library's: needs_exchange says whether they are due, exchange_parts resets their part bookkeeping.
inline int set_shard_parts(AbiState* c, int rank, int world, int parts, int64_t* own_begin, int64_t* own_end) {
    const char* fn = "vamp_sampler_set_shard";
    if (int rc = need_sampler(c, fn)) return rc;
    if (world < 1 || rank < 0 || rank >= world) return bad_arg(fn, "bad rank/world");
    if (parts < 1 || parts > 64) return bad_arg(fn, "parts must be in 1..64");
    if (c->n_regions != 1) return bad_arg(fn, "walker sharding is for single-region contexts (shard regions across devices otherwise)");
    if (c->comm && (world != c->comm_world || rank != c->comm_rank))
        return bad_arg(fn, "rank/world differ from the communicator's (vamp_comm_init_rank)");
    plan::ShardPlan sp;
    {
        const std::string err = plan::plan_shard(c->W, c->split_block, rank, world, parts, sp);
        if (!err.empty()) return bad_arg(fn, err);
    }
    c->shard_rank = rank;
    c->shard_world = world;
    c->shard_parts = parts;
    c->part_slots = sp.part_slots;
    c->part_stride = sp.part_stride;
    c->slot_begin = sp.slot_begin;
    c->slot_end = c->slot_begin + c->part_slots;      // of part 0
    c->exchange = false;
    for (int p = 0; p < parts; ++p) {
        if (own_begin) own_begin[p] = sp.own_begin[p];
        if (own_end) own_end[p] = sp.own_end[p];
    }
    return VAMP_OK;
}
inline bool needs_exchange(const AbiState* c) { return c->shard_world > 1 || c->comm; }
// doubles of the exchange buffers of every part: the movers in slot order, position + lnprob per row; sent by this
// rank, and gathered from all ranks
inline size_t exchange_send_doubles(const AbiState* c) { return plan::exchange_send_doubles(c->shard_parts, c->part_slots, c->regions_h[0].D); }
inline size_t exchange_recv_doubles(const AbiState* c) {
    return plan::exchange_recv_doubles(c->shard_parts, c->shard_world, c->part_slots, c->regions_h[0].D);
}
inline void exchange_parts(AbiState* c) {
    c->part_step.assign(c->shard_parts, 0u);
    c->part_half.assign(c->shard_parts, 0);
}
// doubles of one part's rows: sent by this rank (all = false), or gathered from all ranks
inline size_t part_doubles(const AbiState* c, bool all) {
    return (size_t)(all ? c->shard_world : 1) * c->part_slots * (c->regions_h[0].D + 1);
}

inline int check_half_step(const AbiState* c, int half) {
    if (int rc = need_sampler(c, "vamp_sampler_half_step")) return rc;
    return (half == 0 || half == 1) ? VAMP_OK : bad_arg("vamp_sampler_half_step", "half must be 0 or 1");
}
inline int check_half_step_part(const AbiState* c, int half, int part) {
    const char* fn = "vamp_sampler_half_step_part";
    if (int rc = need_sampler(c, fn)) return rc;
    if (half != 0 && half != 1) return bad_arg(fn, "half must be 0 or 1");
    if (part < 0 || part >= c->shard_parts) return bad_arg(fn, "no such part");
    if (c->comm && c->exchange)
        return bad_state(fn, "with a communicator the exchange is part of vamp_sampler_half_step / vamp_sampler_run");
    return VAMP_OK;
}
// host-supplied draws: a wild index would be an out-of-bounds access of the state
inline int check_half_step_ext(const AbiState* c, int region, long long n, const int32_t* active_idx, const int32_t* partner_idx,
                               const double* zz, const double* logu) {
    const char* fn = "vamp_sampler_half_step_ext";
    if (!c || !active_idx || !partner_idx || !zz || !logu) return bad_arg(fn, "NULL argument");
    if (int rc = need_sampler(c, fn)) return rc;
    if (int rc = need_region(c, region, fn)) return rc;
    if (n <= 0 || n > c->W) return bad_arg(fn, "bad n");
    std::vector<char> is_active(c->W, 0);
    for (long long i = 0; i < n; ++i) {
        if (active_idx[i] < 0 || active_idx[i] >= c->W || partner_idx[i] < 0 || partner_idx[i] >= c->W)
            return bad_arg(fn, "walker index out of range");
        if (is_active[active_idx[i]]) return bad_arg(fn, "duplicate active walker");
        is_active[active_idx[i]] = 1;
        if (!(zz[i] > 0.0)) return bad_arg(fn, "stretch factor must be positive");
    }
    for (long long i = 0; i < n; ++i)
        if (is_active[partner_idx[i]]) return bad_arg(fn, "partner must belong to the frozen complement");
    return VAMP_OK;
}
// vamp_sampler_run (dev = false) and vamp_sampler_run_dev (dev = true, which also takes the shard rule)
inline int check_run(const AbiState* c, bool dev, long long n_steps, int thin) {
    const char* fn = dev ? "vamp_sampler_run_dev" : "vamp_sampler_run";
    if (int rc = need_sampler(c, fn)) return rc;
    if (n_steps < 0 || thin < 1) return bad_arg(fn, "n_steps >= 0 and thin >= 1 required");
    if (dev && c->shard_world != 1 && !(c->comm && c->exchange))
        return bad_state(fn, "a sharded context without a communicator is stepped by the host (half_step_part + pack_get / scatter_put)");
    return VAMP_OK;
}
inline int check_set_state(const AbiState* c, const double* theta, const double* lnprob, long long step) {
    if (!c || !theta || !lnprob) return bad_arg("vamp_sampler_set_state", "NULL argument");
    if (int rc = need_sampler(c, "vamp_sampler_set_state")) return rc;
    return step >= 0 ? VAMP_OK : bad_arg("vamp_sampler_set_state", "step must be >= 0");
}

// ---- walker-sharded runs --------------------------------------------------------------------------------------------
inline int check_unique_id(const char* id) { return id ? VAMP_OK : bad_arg("vamp_comm_unique_id", "id is NULL"); }
inline int check_comm_init_rank(const AbiState* c, const char* id, int rank, int world) {
    const char* fn = "vamp_comm_init_rank";
    if (!c || !id) return bad_arg(fn, "NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return bad_arg(fn, "bad rank/world");
    if (c->comm) return bad_state(fn, "the context already has a communicator");
    // either order of vamp_sampler_set_shard_parts and vamp_comm_init_rank is accepted, but they must agree
    if (c->sampler_ready && (c->shard_world != 1 || c->exchange) && (c->shard_world != world || c->shard_rank != rank))
        return bad_arg(fn, "rank/world differ from the shard already set (vamp_sampler_set_shard_parts)");
    return VAMP_OK;
}
// the communicator is in place; true: the shard came first, and its exchange buffers (a single-rank shard has none yet)
// are due now
inline bool join_comm(AbiState* c, int rank, int world) {
    c->comm = true;
    c->comm_rank = rank;
    c->comm_world = world;
    return c->sampler_ready && c->n_regions == 1 && c->part_slots > 0;
}
inline void leave_comm(AbiState* c) {
    c->comm = false;
    c->comm_rank = 0;
    c->comm_world = 1;
}
inline int check_comm_info(const AbiState* c) {
    if (int rc = need_ctx(c, "vamp_comm_info")) return rc;
    return c->comm ? VAMP_OK : bad_state("vamp_comm_info", "the context has no communicator (vamp_comm_init_rank)");
}
inline int check_comm_library(const char* path, long long capacity) {
    return (!path || capacity < 2) ? bad_arg("vamp_comm_library", "no room for a path") : VAMP_OK;
}
// vamp_sampler_pack_get (scatter = false) and vamp_sampler_scatter_put (scatter = true)
inline int check_exchange_rows(const AbiState* c, bool scatter, int part, const double* rows) {
    const char* fn = scatter ? "vamp_sampler_scatter_put" : "vamp_sampler_pack_get";
    if (!c || !rows) return bad_arg(fn, "NULL argument");
    if (!c->sampler_ready || !c->exchange) return bad_state(fn, "no sharded sampler (vamp_sampler_set_shard_parts with world > 1)");
    return (part >= 0 && part < c->shard_parts) ? VAMP_OK : bad_arg(fn, "no such part");
}

}  // namespace vamp
