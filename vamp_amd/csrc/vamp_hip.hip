// vamp_hip.hip -- MI355X (gfx950) kernels + C ABI for VAMP's MCMC hot path.
//
// Replaces, below the Python surface of class VPfit (reference vamp_1.0/vpfits.py:33):
//   * the per-proposal evaluation of the PyMC model graph -- profile closures
//     (vpfits.py:254-260, 299-305), `total` = Tau2flux(sum(profiles)) (vpfits.py:334-336,
//     physics.py:105), the observed Normal likelihood (vpfits.py:39,341) and the priors
//     (vpfits.py:239-252, 283-297);
//   * the sampler loop of mcmc_fit / find_bic (vpfits.py:361-395, 420-425), by the stretch move
//     of Goodman & Weare (2010) with emcee's red/blue semantics.
//
// Execution shape (struct Pack): a walker is served by one 64-lane wavefront, by a quarter of one
// (short regions), or by a 4-wavefront workgroup whose wavefronts take every 4th 256-pixel tile
// (long regions: the headline).
//   stage   lanes 0..K-1 turn the walker's parameters into per-line records in LDS
//           (centroid, x-scale, damping y, tau scale, pole factor) and all lanes fill the per-line
//           table 1/(u_n^2 + y^2) of the near-axis Voigt rule; priors are summed here.  A
//           workgroup then builds the Taylor tables of the line cores (struct LineTables).
//   sweep   lane l takes pixels l, l+64, ... of a tile: coalesced 512-byte reads of x / flux /
//           1/sigma (shared by every walker -> L2/MALL resident); near lines are evaluated per
//           pixel, all distant lines of the tile through ONE Chebyshev interpolant (ff_*);
//           tau in registers, flux = exp(-tau), chi^2 partial per lane.
//   reduce  xor-shuffle tree over the wavefront (+ LDS across the workgroup); lane 0 owns the result.
//   move    (sampler kernel) proposal q = c - (c - s) z is formed in LDS before `stage`, and the
//           accept test / state update follow `reduce` in the same launch.
// Kernels: k_lnprob / k_half_step (one launch per evaluation / per half-step of the stretch move), k_draws (the draws
// of packed launches), k_run_resident (small ensembles: one workgroup per region runs the region's WHOLE step loop),
// k_map_search (one workgroup per region runs its WHOLE Nelder-Mead MAP search, vpfits.py:352-358, 426), k_model,
// k_scatter_rows (walker-sharded runs), k_wofz / k_line_records (test hooks).
// No MFMA (nothing here is a contraction), no atomics, no inter-workgroup communication.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/vamp_hip.h"
#include "abi_state.hpp"
#include "draws.hpp"
#include "host_plan.hpp"
#include "map_search.hpp"
#include "voigt_math.hpp"
#include "ff_predicates.hpp"
#include "ff_moments.hpp"

#ifndef VAMP_EARLY_LOADS
#define VAMP_EARLY_LOADS 1
#endif
#ifndef VAMP_BLEND_PASS_LINES
#define VAMP_BLEND_PASS_LINES 4
#endif
#ifndef VAMP_MID_MIN_K
#define VAMP_MID_MIN_K 3
#endif
#ifndef VAMP_MID_MIN_P
#define VAMP_MID_MIN_P 96
#endif
#ifndef VAMP_X_PREFETCH
#define VAMP_X_PREFETCH 0
#endif

#ifndef VAMP_MIN_WAVES
#define VAMP_MIN_WAVES 3
#endif
#ifndef VAMP_EARLY_LNP
#define VAMP_EARLY_LNP 1
#endif
#ifndef VAMP_SR_EARLY
#define VAMP_SR_EARLY 0
#endif
#ifndef VAMP_XCD_MAP
#define VAMP_XCD_MAP 0        // region -> XCD mapping of multi-region launches: measured, off (k_half_step; profiles/r04_d_xcd_mapping.txt)
#endif
#ifndef VAMP_WIDE_NODES
#define VAMP_WIDE_NODES 1      // lines far wider than a tile join the tile's interpolant (sweep_range_ff)
#endif
#ifndef VAMP_LPT
#define VAMP_LPT 1             // small ensembles: the regions of a launch class in order of decreasing work
#endif
#ifndef VAMP_FLUX_EXP_DROP
#define VAMP_FLUX_EXP_DROP 2   // far-field sweep: exp(-tau) of the model flux by the degree-11 kernel (6e-15) instead of degree 13
#endif
#ifndef VAMP_FF_R2_M4
#define VAMP_FF_R2_M4 100.0    // far-field node values: below this |z|^2 the 6-level fraction, ...
#define VAMP_FF_R2_M3 300.0    // ... below this the 4-level, ...
#define VAMP_FF_R2_M2 2000.0   // ... below this the 3-level, beyond it the 2-level one
#endif
#ifndef VAMP_F32_FAR_CORE
#define VAMP_F32_FAR_CORE 1    // fp32 far field: far = outside the Gaussian core (|z|^2 >= VAMP_MID_Z2) instead of outside |z| < 8
#endif
#ifndef VAMP_CORE_FASTPATH
#define VAMP_CORE_FASTPATH 1   // tile_voigt: a wavefront wholly inside |z| < 8 of a line evaluates its pixels in straight-line code
#endif
#ifndef VAMP_MID_NODES
#define VAMP_MID_NODES 1       // lines >= FF_DIST half-widths beyond a tile whose |z| < 8 zone still reaches into it join the interpolant too ...
#endif
#ifndef VAMP_MID_Z2
#define VAMP_MID_Z2 30.25      // ... when the whole tile is outside |z|^2 < this (e^{-30.25} = 7e-14 of the line's peak)
#endif
#ifndef VAMP_WIDE_MAX
#define VAMP_WIDE_MAX 0.75     // ... when the tile's half-width is at most this many units of the line's z.  Worst relative lnprob
#endif                         // error at the switch on well-fitted data at S/N 200 (tests/wide_probe.py, profiles/r04_e_wide_lines.txt):
                               // 0.5: 4e-16, 0.75: 4e-14, 1.0: 1.2e-12 (3e-11 with amplitudes of 20), 1.25: 7e-11; the bar is 1e-9
#ifndef VAMP_F32_LEAN_STAGE
#define VAMP_F32_LEAN_STAGE 1
#endif
#ifndef VAMP_TILE_MOMENTS
#define VAMP_TILE_MOMENTS 2    // fp64 far-field loop: chi^2 of a tile without a near line from the context's data moments (ff_moments.hpp):
#endif                         // 2: a quadratic form in the 16 node values; 1: in the four series of the tile; 0: every tile pixel by pixel
#ifndef VAMP_NODE_PASS
#define VAMP_NODE_PASS 1       // fp64 far-field loop: the node values of a full batch of four tiles line by line, lane = (tile, node)
#endif                         // (ff_node_pass, sweep_range_ff_np); 0: tile by tile from the tiles' lists (ff_node_sums)
#ifndef VAMP_NP_CLASS_RUNS
#define VAMP_NP_CLASS_RUNS 1   // node pass: one counted loop of pairs per depth, its constants read once ahead of it, the records of
#endif                         // a pair read by every lane one pair ahead (vamp::np_pair_order); 0: depth and pair chosen inside one loop
#ifndef VAMP_DEAL_ADJ
#define VAMP_DEAL_ADJ 1        // node pass: a full batch is four ADJACENT tiles, class p of PARTS takes tiles 16 m + 4 p .. 16 m + 4 p + 3 of
#endif                         // every whole group of 16 tiles; 0: tiles p, p + 4, p + 8, p + 12.  What no group holds is dealt p, p + 4, ..
#ifndef VAMP_SUPER_NODES
#define VAMP_SUPER_NODES 1     // node pass (needs VAMP_DEAL_ADJ): the lines distant from all four tiles of a batch (vamp::ff_super_distant) once at
#endif                         // the 16 nodes of the batch's super-tile, eight lines per iteration, and interpolated to the tiles' nodes (ff_super_pass),
                               // inside the one loop of the walkers without a guard bit, behind one scalar branch per batch that a walker with a line
                               // wide for every tile does not take (profiles/super_nodes_on_ab.txt; the forms before it: profiles/super_nodes_ab.txt)
#ifndef VAMP_TAB_PAIR
#define VAMP_TAB_PAIR 0        // in-zone near lines: the Taylor table for two pixels of a lane at a time (table_eval2): measured, off
#endif                         // (+0.4 % on the headline; profiles/tile_loop_waits_ab.txt); 0: one by one
#ifndef VAMP_TILE_HEAD
#define VAMP_TILE_HEAD 0       // fp64 far-field loop: a tile's abscissae requested after the test that it is done from its moments:
#endif                         // measured, off (-0.2 %, inside the runs' spread; profiles/tile_loop_waits_ab.txt)
namespace {

constexpr int KMAX = 16;                       // lines per region of the fast shapes (far field, Taylor tables, packing)
constexpr int KMAX_ALL = VAMP_MAX_COMPONENTS;  // lines per region of the ABI: 17 .. 32 run the plain shape PackXL
static_assert(KMAX_ALL >= KMAX && KMAX_ALL < 64, "lane k stages line k; one spare lane for sd");
constexpr int WAVES_PER_BLOCK = 4;
constexpr long long PACK_MIN_WALKERS = 16384;   // movers per launch from which the packed shapes fill the chip
constexpr int RES_MAX_MOVERS = 128;             // movers per half-step (W / 2) a resident workgroup serves; also: "a small ensemble"
#ifndef VAMP_RES_WAVES
#define VAMP_RES_WAVES 8
#endif
constexpr int RES_MAX_WAVES = VAMP_RES_WAVES;   // compute wavefronts of a resident workgroup (+ the one that draws)
constexpr int BLOCK = 64 * WAVES_PER_BLOCK;
constexpr int DMAX = 4 * KMAX_ALL + 1;
// automatic choice of a 4-wave workgroup per walker (shared Taylor tables of the line cores, see
// LineTables): regions that give every wave >= 2 tiles.  The choice must not depend on the launch
// size: a shard of an ensemble has to run the same arithmetic as the whole ensemble on one GPU.
#ifndef VAMP_SPLIT_MAX_WALKERS
#define VAMP_SPLIT_MAX_WALKERS (1ll << 62)
#endif
constexpr long long SPLIT_MAX_WALKERS = VAMP_SPLIT_MAX_WALKERS;

constexpr double C_LIGHT = 2.98e8;     // physics.py:3 (the reference's value)
constexpr double SIGMA0 = 0.0263;      // physics.py:4
constexpr double SQRT_LN2 = 0.83255461115769775635;
constexpr double SQRT_PI = 1.77245385090551602730;
constexpr double FWHM_PER_SIGMA = 2.35482004503094938202;   // 2 sqrt(2 ln 2), vpfits.py:88,326
constexpr double NEG_INF = -__builtin_huge_val();

using vamp::RegionDev;        // one region (one posterior): abi_state.hpp

struct LineRec {           // per (walker, component), lives in LDS
    double c;              // centroid
    double s;              // Voigt: 2 sqrt(ln2)/G ; Gauss: 1/sigma
    double y;              // Voigt: L sqrt(ln2)/G
    double amp;            // Voigt: A y (tau_k = A y sqrt(pi) H: the evaluators return sqrt(pi) H) ; Gauss: A
    double pole;           // core_pole_factor(y)
    double hy;             // core_hy(y)
    double xcap;           // +inf, or X_FAR when one tile of pixels spans > 16 units of |z| (narrow line)
    double w8, w25;        // half-widths, in x, of |z|^2 < 64 and |z|^2 < 625 around the centre (far-field classification)
    double wmid;           // ... and of |z|^2 < VAMP_MID_Z2 (the Gaussian core's reach)
};

// Packing of walkers onto wavefronts.  LPW lanes serve one walker (SUBS = 64/LPW walkers share a
// wave); KCAP bounds the lines per walker and so the LDS footprint.  <64,16> is the headline shape
// (thousands of pixels per region); <16,8> serves the 9..478-pixel regions of real spectra, where
// one walker cannot fill a wave and the per-walker fixed work (staging, draws, reduction) dominates.
//
// SPLIT: the full tiles of a region are dealt round-robin into PARTS classes and chi^2 is summed
// class by class (so the summation order does not depend on the packing).  SPLIT = false: one wavefront
// sweeps all classes of its walker.  SPLIT = true: the workgroup serves ONE walker and wavefront j
// sweeps class j -- four times as many, four times shorter wavefronts, for launches with too few
// walkers to fill 256 CUs evenly (a shard of the headline ensemble on one of 8 GPUs is 4096
// walkers per half-step = 1.3 wavefronts per SIMD slot; the drain at the end of a launch costs
// about half a wavefront lifetime).  The group shares one set of line records and tables.
#ifndef VAMP_PARTS
#define VAMP_PARTS 4
#endif
constexpr int PARTS = VAMP_PARTS;
template <int KCAP, bool OWN_DTAB> struct WalkerLds;
// Timing-only builds (-DVAMP_STAMPS, tools/stamps.py): the first lane of workgroup 0 records (tag, shader clock) pairs
// along one walker's path through a half-step -- where a latency-bound wavefront's time goes
#ifdef VAMP_STAMPS
__device__ unsigned long long g_stamps[2 * 8192];
__device__ unsigned int g_stamp_n;
#define VAMP_STAMP(tag)                                                                          \
    do {                                                                                         \
        if (blockIdx.x == 0 && threadIdx.x == 0) {                                               \
            const unsigned int n_ = g_stamp_n;                                                   \
            if (n_ < 8192) { g_stamps[2 * n_] = (tag); g_stamps[2 * n_ + 1] = __builtin_amdgcn_s_memtime(); g_stamp_n = n_ + 1; } \
        }                                                                                        \
    } while (0)
#define VAMP_STAMP_AFTER(tag, v) do { asm volatile("" :: "v"(v)); VAMP_STAMP(tag); } while (0)     // once `v` has arrived
#else
#define VAMP_STAMP(tag) do {} while (0)
#define VAMP_STAMP_AFTER(tag, v) do {} while (0)
#endif
#ifndef VAMP_SPLIT_WAVES
#define VAMP_SPLIT_WAVES 4
#endif
#ifndef VAMP_SPLIT_WAVES_F32
#define VAMP_SPLIT_WAVES_F32 4
#endif
#ifndef VAMP_F32_TABLES
#define VAMP_F32_TABLES 1
#endif
template <int LPW_, int KCAP_, bool TAIL_, int WPB_, bool SPLIT_ = false, bool TABS_ = SPLIT_, bool FF_ = (LPW_ == 64)>
struct Pack {
    static constexpr int LPW = LPW_, KCAP = KCAP_, SUBS = 64 / LPW_;
    static constexpr bool TAIL = TAIL_;     // false: every region is a whole number of full tiles
    static constexpr bool SPLIT = SPLIT_;
    static constexpr bool TABS = TABS_;     // per-walker Taylor tables of the line cores (fp64 Voigt)
    static constexpr bool FF = FF_;         // far-field interpolant in full tiles
    static constexpr int WPB = WPB_;        // wavefronts per workgroup
    static constexpr int THREADS = 64 * WPB_;
    static constexpr int WALKERS_PER_BLOCK = SPLIT_ ? 1 : WPB_ * SUBS;
    // wavefronts per SIMD the register allocation aims for (MIN_WAVES below): 3 (<= 168 VGPRs), 4 (128 VGPRs,
    // 40 KB of LDS) for the workgroup-per-walker shape with the far field, 2 for a blend shape with every
    // line's tables resident
    // the blend shape keeps the Taylor tables of only LINES_PER_PASS lines in LDS at a time (0: of all
    // KCAP lines) and sweeps its pixels once per pass with the optical depths held in registers:
    // 9 KB instead of 18 KB of tables per walker, 3 instead of 1.7 wavefronts per SIMD
    static constexpr int LINES_PER_PASS = (SPLIT_ && TABS_ && !FF_ && WPB_ == 1) ? VAMP_BLEND_PASS_LINES : 0;
    static constexpr int TAB_LINES = LINES_PER_PASS > 0 ? LINES_PER_PASS : KCAP_;
    // the workgroup-per-walker shape with every line's tables resident needs the near-axis tables (dtab) only
    // until the Taylor rows are built from them: they live in the tail of the tables' own space (5.6 KB
    // less LDS: 39.7 KB per workgroup)
    static constexpr bool DTAB_IN_TABLES = SPLIT_ && TABS_ && FF_;
    using Lds = WalkerLds<KCAP_, !DTAB_IN_TABLES>;
    static constexpr int MIN_WAVES = (SPLIT_ && TABS_ && !FF_ && LINES_PER_PASS == 0) ? 2 : DTAB_IN_TABLES ? VAMP_SPLIT_WAVES : VAMP_MIN_WAVES;
    static_assert(!SPLIT_ || (LPW_ == 64 && (WPB_ == PARTS || !FF_) && WPB_ <= PARTS),
                  "a split workgroup is PARTS wavefronts on one walker (tile classes), or up to PARTS wavefronts without far field (contiguous shares)");
};
using PackWide = Pack<64, KMAX, true, WAVES_PER_BLOCK>;
using PackWideFull = Pack<64, KMAX, false, WAVES_PER_BLOCK>;   // the headline shape: no tail code
using PackSplit = Pack<64, KMAX, true, PARTS, true>;
using PackSplitFull = Pack<64, KMAX, false, PARTS, true>;
// 8 walkers x 3.7 KB of LDS per 128-thread workgroup: 5 workgroups (10 waves) per CU
using PackSmall = Pack<16, 8, true, 2>;
// the same for regions of one or two lines (most regions of a real spectrum): 0.9 KB instead of
// 3.7 KB of LDS per walker, so that registers, not LDS, set the occupancy
#ifndef VAMP_SMALL2_WAVES
#define VAMP_SMALL2_WAVES 2
#endif
#ifndef VAMP_SMALL2_LANES
#define VAMP_SMALL2_LANES 8
#endif
using PackSmall2 = Pack<VAMP_SMALL2_LANES, 2, true, VAMP_SMALL2_WAVES>;
// one walker per small workgroup WITH its own Taylor tables (<= 8 lines: 18 KB + 3.7 KB of LDS),
// no far field; the group's wavefronts share the staging and take contiguous shares of the pixels: the blended regions of real spectra (3..8 lines,
// ~100..500 px), where every pixel lies in some line's core and the near-axis rule (~190 issue
// slots per evaluation against ~40 through a table) is the whole cost
#ifndef VAMP_MID_WAVES
#define VAMP_MID_WAVES 1
#endif
#ifndef VAMP_MID_PREDRAW
#define VAMP_MID_PREDRAW 1
#endif
using PackMid = Pack<64, 8, true, VAMP_MID_WAVES, true, true, false>;
// regions of 17 .. 32 lines (the reference sets no limit, vpspectrum.py:287-294): one walker per wavefront, every
// line evaluated per pixel, no far field and no tables; 15 KB of LDS per walker, two walkers per workgroup
using PackXL = Pack<64, KMAX_ALL, true, 2, false, false, false>;

constexpr int FF_NODES = 16;          // Chebyshev nodes of the far-field interpolant of one tile
constexpr int FF_BATCH = 4;           // tiles of a wavefront whose lines are classified in one 64-lane pass
#ifndef VAMP_FF_DIST
#define VAMP_FF_DIST 2.0        // (round 4: was 4.  The series reproduce a wing from 2 half-widths to 3e-11 of ITS value there,
                                //  tests/test_ff_matrix.py; on well-fitted data with strong damped wings the log-posterior moves
                                //  by 6e-15, tests/ff_probe.py; one tile fewer per side where a narrow line is near: -2.5 %)
#endif
constexpr double FF_DIST = VAMP_FF_DIST;   // a line is "far" from a tile when it lies >= FF_DIST half-widths beyond its edge
#include "ff_matrix.inc"               // FF_M, FF_DEG, FF_ROWS, FF_MAT (tools/gen_ff_matrix.py)
#include "ff_matrix32.inc"             // FF32_M, FF32_NODES, FF32_DEG, FF32_ROWS, FF32_MAT: the fp32 contexts' 8-node form

template <int KCAP, bool OWN_DTAB = true>
struct WalkerLds {
    double theta[4 * KCAP + 4];
    LineRec line[KCAP];
    double dtab[OWN_DTAB ? KCAP : 1][vamp::DTAB_N];     // !OWN_DTAB: in the tail of the Taylor tables (Pack::DTAB_IN_TABLES)
    float linef[KCAP][4];  // fp32 path: c, s, y, amp
};
struct alignas(16) TileScratch {   // per wavefront: far-field working set of the tile in flight
    double coef[FF_ROWS];   // optical depth of the far lines at the tile's 16 Chebyshev nodes, then (every lane has
                            // read the node values by then) the tile's four local power series, one per quarter,
                            // 14 coefficients each; fp32 contexts store those as floats in the same space
    // the lists of the FF_BATCH tiles classified together (ff_classify_batch), one row per tile, as line indices in
    // bytes: the same 128 B as one tile's two lists of ints; a reader scales the index by its record size with a
    // full-rate 24-bit multiply
    unsigned char farlist[FF_BATCH][KMAX];    // lines treated through the far field: deep ones first, then the others, each in line order
    unsigned char widelist[FF_BATCH][KMAX];   // near lines far WIDER than the tile, or between far and near (fp64 tables shape), in line order
};
static_assert(KMAX == 16 && FF_BATCH * KMAX == 64, "lane 16 j + k classifies line k against tile j of a batch");
// Taylor tables of the near-axis zone of every line of ONE walker (voigt_math.hpp): 28 KiB, which
// only a workgroup that serves a single walker can afford (4 workgroups per CU).
template <int NDBL>
struct alignas(16) LineTables { double a[NDBL]; };
template <bool F32, int MODE, class PK>
constexpr bool use_tables() { return PK::TABS && !F32 && MODE != VAMP_GAUSS3; }
// fp32 contexts, workgroup-per-walker shape: the line cores through single-precision Taylor rows (voigt_math.hpp,
// TAB32_*) instead of Humlicek's regions III / IV.  The space holds the rows of all KMAX lines (8 KB) followed by
// the near-axis tables (5.6 KB of doubles) the rows' centre values are computed from.
template <bool F32, int MODE, class PK>
constexpr bool use_tables32() { return VAMP_F32_TABLES && PK::DTAB_IN_TABLES && F32 && MODE != VAMP_GAUSS3; }
constexpr int TAB32_DOUBLES = KMAX * vamp::TAB32_LINE / 2;       // the float rows, counted in doubles
// fp32 contexts, blend shape (one wavefront per walker, <= 8 lines over <= 512 pixels): the fp32 rows of ALL its
// lines resident (512 B per line), built from the walker's own near-axis tables
template <bool F32, int MODE, class PK>
constexpr bool use_blend32() { return VAMP_F32_TABLES && F32 && PK::LINES_PER_PASS > 0 && MODE != VAMP_GAUSS3; }
template <bool F32, int MODE, class PK>
constexpr int table_doubles() {
    return use_tables<F32, MODE, PK>() ? PK::TAB_LINES * vamp::TAB_LINE
           : use_tables32<F32, MODE, PK>() ? TAB32_DOUBLES + KMAX * vamp::DTAB_N
           : use_blend32<F32, MODE, PK>() ? PK::KCAP * vamp::TAB32_LINE / 2 : 2;
}
// wavefronts per SIMD the register allocation aims for: fp32 instructions issue in 2 cycles on a SIMD but one
// wavefront can issue only every 4, so the fp32 form of the workgroup-per-walker shape wants MORE resident
// wavefronts than the fp64 one (it has no Taylor tables: 12 KB of LDS per workgroup)
template <bool F32, class PK>
constexpr int min_waves() { return (F32 && PK::DTAB_IN_TABLES) ? VAMP_SPLIT_WAVES_F32 : PK::MIN_WAVES; }

// the near-axis table of line k as the evaluators want it (unused by the table look-ups; not addressable
// through L when it lives in the tables' space)
template <class PK>
__device__ __forceinline__ const double* dtab_row(const typename PK::Lds& L, int k) {
    if constexpr (PK::DTAB_IN_TABLES) return nullptr;
    else return L.dtab[k];
}

// barrier over the lanes that stage and sweep one walker together
// (a split group of ONE wavefront -- the blend shape -- synchronises like any single wavefront: its lanes' LDS
//  operations execute in program order, so the device-resident step loop can run several such walkers, one per
//  wavefront, in one workgroup)
template <class PK>
__device__ __forceinline__ void group_barrier() {
    if constexpr (PK::SPLIT && PK::WPB > 1) __syncthreads();
    else __builtin_amdgcn_wave_barrier();
}
using WaveLds = WalkerLds<KMAX_ALL, true>;  // the one-walker-per-wavefront kernels (k_model, k_line_records): = PackXL::Lds

// ---------------------------------------------------------------------------------------
// wave helpers
// ---------------------------------------------------------------------------------------
template <int LPW = 64>
__device__ __forceinline__ double wave_sum(double v) {      // sum over the LPW lanes of one walker
#pragma unroll
    for (int off = LPW / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// largest value of the 16 lanes of a lane's row, on every lane of the row: row rotations in the data path (DPP), no lane
// addresses in registers -- for use inside the tile loop, which has none to spare
template <int N>
__device__ __forceinline__ double row_ror(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x120 + N, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x120 + N, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// the lane's index in its wavefront, computed where it is called (two instructions the compiler neither hoists nor
// keeps): for a loop that may hold nothing a lane derives from its index across its iterations
__device__ __forceinline__ int lane_here() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
__device__ __forceinline__ double row16_max(double v) {
    v = fmax(v, row_ror<8>(v));
    v = fmax(v, row_ror<4>(v));
    v = fmax(v, row_ror<2>(v));
    return fmax(v, row_ror<1>(v));
}

// vpfits.py:239-244: -inf for v < 0, else log(v*exp(-v)).  For v <= 700 that is log(v) - v to an
// ulp of the result (one transcendental instead of two); beyond, exp(-v) leaves the normal range
// and the reference's literal form -- which ends in log(0) = -inf from v ~ 745 -- is kept.
__device__ __forceinline__ double xexp_logp(double v) {
    if (!(v >= 0.0) || !isfinite(v)) return NEG_INF;
    if (v <= 700.0) return log(v) - v;
    return log(v * exp(-v));
}
// the same in fp32 contexts: the logarithm in single precision (~1e-7 of a term of order 1 in a log-posterior whose
// chi^2 carries W4's 1e-4; the stated tolerance is 1e-3 of chi^2), v itself subtracted in double
__device__ __forceinline__ double xexp_logp32(double v) {
    if (!(v >= 0.0) || !isfinite(v)) return NEG_INF;
    if (v <= 700.0) return (double)__logf((float)v) - v;
    return log(v * exp(-v));
}
__device__ __forceinline__ double uniform_logp(double v, double lo, double hi, double lp) {
    return (v >= lo && v <= hi) ? lp : NEG_INF;
}

// The two rare cases of the far-field node evaluation (ff_eval2) are decided by a walker's lines, not by the tile:
//   tiny:  y < Y_TINY -- the fractions miss e^{-x^2}, which ff_eval2 adds back;
//   reach: the line is so narrow that a node of the region can lie beyond X_FAR in its z, where ff_eval2 clamps the
//          argument and patches the value.  Every node lies between the region's first and last abscissa (the grid is
//          monotonic, vamp_set_regions checks it), |x - c| is largest at one of the two ends wherever c lies, and rounding
//          is monotonic, so s max(|x_first - c|, |x_last - c|) bounds every node's X as computed; NaN sets the bit.
// One line with either bit sends its walker through the guarded copy of the tile loop -- today's code -- and a walker
// without runs the copy that has neither the clamps nor the votes (sweep_class).
__device__ __forceinline__ void ff_guard_bits(const LineRec& rec, double x_first, double x_last, bool& tiny, bool& reach) {
    tiny = !(rec.y >= vamp::Y_TINY);
    reach = !(rec.s * fmax(fabs(x_first - rec.c), fabs(x_last - rec.c)) <= vamp::X_FAR);
}

// Turn theta (in LDS) into line records + prior.  Returns log-prior on every lane.
// MODE is a compile-time parameter: one specialised kernel per parameterisation, no mode
// branches in the staging code or in the pixel loop.
// FFG (ff_guard_bits): the walker's two guard bits of the fp64 far-field node evaluation, from the region's abscissae xr.
template <int MODE, class PK = PackWide, bool TAB = false, bool TAB32 = false, bool DT32 = false, bool FFG = false>
__device__ __forceinline__ double stage_lines(const RegionDev& R, typename PK::Lds& L, int lane, bool want_f32, int part,
                                              double* tab = nullptr, const double* __restrict__ xr = nullptr) {
    // `lane` is the lane index inside the walker's group (0 .. LPW-1).  In a split workgroup
    // (`part` = wavefront index) the FIRST wavefront evaluates the records and the prior and leaves the
    // prior in a spare slot of the parameter block for the others (each needs it to decide whether to
    // sweep); the per-line tables are filled by all 256 threads.  (All four used to evaluate them: the
    // kernel is bound by VALU throughput, and the staging -- divisions, square roots, a logarithm per
    // line -- was 3 % of its instructions three times over.)
    const bool writer = !PK::SPLIT || part == 0;
    constexpr int LP_SLOT = 4 * PK::KCAP + 3;       // theta holds at most 4 KCAP + 1 parameters
    constexpr int WIDE_SLOT = 4 * PK::KCAP + 2;     // far-field shapes: bit k set = line k is far wider than a tile (ff_wide_nodes);
                                                    // bits 16, 17: the guard bits
    bool my_wide = false, my_tiny = false, my_reach = false;
    double lp = 0.0;
    const int K = R.K;
    constexpr int Q = (MODE == VAMP_VOIGT4) ? 4 : 3;
    // fp32 contexts (VAMP_F32_LEAN_STAGE): the amplitude prior's logarithm in single precision, and no pole factor /
    // h y where no near-axis table will be built from them (Humlicek's W4 reads neither) -- the staging is ~1/4 of a
    // short region's half-step in fp32 (profiles/r04_c_small_ensembles.txt, stamps 2 -> 3)
    const bool lean = VAMP_F32_LEAN_STAGE && want_f32;
    const bool need_core = !(VAMP_F32_LEAN_STAGE && want_f32 && !TAB32 && !DT32);
    if (lane < K && writer) {
        const double* t = &L.theta[Q * lane];
        double a, c, Lw = 0.0, G = 0.0, sg = 0.0;
        if constexpr (MODE == VAMP_GAUSS3) {
            a = t[0]; c = t[1]; sg = t[2];
            lp = (lean ? xexp_logp32(a) : xexp_logp(a)) + uniform_logp(c, R.c_lo, R.c_hi, R.lp_c) + uniform_logp(sg, 0.0, R.w_max, R.lp_w);
        } else if constexpr (MODE == VAMP_VOIGT4) {
            a = t[0]; c = t[1]; Lw = t[2]; G = t[3];
            lp = (lean ? xexp_logp32(a) : xexp_logp(a)) + uniform_logp(c, R.c_lo, R.c_hi, R.lp_c) +
                 uniform_logp(Lw, 0.0, R.w_max, R.lp_w) + uniform_logp(G, 0.0, R.w_max, R.lp_w);
        } else {   // NBZ3: inverse of physics.py:15,27,120,134
            const double sig = t[1] * 1.0e3 * 1.41421356237309514547 / (2.355 * (R.line * 1.0e-10));
            a = t[0] * SIGMA0 / (sig * 2.50662827463100024161);
            c = (C_LIGHT / (R.line * (1.0 + t[2]) * 1.0e-10) - R.x_origin) / R.x_scale;
            G = (sig / R.x_scale) * FWHM_PER_SIGMA;
            Lw = R.l_fixed;
            lp = (lean ? xexp_logp32(a) : xexp_logp(a)) + uniform_logp(c, R.c_lo, R.c_hi, R.lp_c) + uniform_logp(G, 0.0, R.w_max, R.lp_w);
        }
        LineRec rec;
        rec.c = c;
        if constexpr (MODE == VAMP_GAUSS3) {
            rec.s = 1.0 / sg; rec.y = 0.0; rec.amp = a; rec.pole = 0.0; rec.hy = 0.0; rec.xcap = __builtin_huge_val();
            rec.w8 = rec.w25 = rec.wmid = 0.0;
        } else {
            const double rG = vamp::rcp_nr(G);          // one reciprocal for both scales (G = 0 -> inf -> rejected below)
            rec.s = (2.0 * SQRT_LN2) * rG;
            rec.y = (Lw * SQRT_LN2) * rG;
            rec.amp = a * rec.y;
            rec.pole = need_core ? vamp::core_pole_factor(rec.y) : 0.0;
            rec.hy = need_core ? vamp::core_hy(rec.y) : 0.0;
            // packed waves: another walker of the wave may force a deep fraction on this one, so every
            // line is capped there
            rec.xcap = (PK::SUBS == 1 && rec.s * R.tile_span <= 16.0) ? __builtin_huge_val() : vamp::X_FAR;   // NaN -> capped
            if constexpr (PK::FF) {
                rec.w8 = sqrt(fmax(vamp::R2_CORE - rec.y * rec.y, 0.0)) / rec.s;
                rec.w25 = sqrt(fmax(vamp::R2_M3 - rec.y * rec.y, 0.0)) / rec.s;
                rec.wmid = sqrt(fmax(VAMP_MID_Z2 - rec.y * rec.y, 0.0)) / rec.s;
                // half of the region's widest tile is at most VAMP_WIDE_MAX in this line's z: smooth across every tile
                my_wide = VAMP_WIDE_NODES && TAB && rec.s * (0.5 * R.tile_span) <= VAMP_WIDE_MAX;
                if constexpr (FFG) ff_guard_bits(rec, xr[0], xr[R.P - 1], my_tiny, my_reach);
            } else {
                rec.w8 = rec.w25 = rec.wmid = 0.0;
            }
            // a degenerate width (G = 0 or non-finite scale) makes the reference's profile NaN, which
            // its sampler rejects; reject here, before the sweep
            if (!(rec.s < __builtin_huge_val()) || !(rec.y < __builtin_huge_val())) lp = NEG_INF;
        }
        if (writer) L.line[lane] = rec;
        if (want_f32 && writer) {
            L.linef[lane][0] = (float)rec.c; L.linef[lane][1] = (float)rec.s;
            L.linef[lane][2] = (float)rec.y;
            L.linef[lane][3] = (float)(MODE == VAMP_GAUSS3 ? rec.amp : rec.amp * SQRT_PI);   // W4 returns H itself
        }
    }
    if constexpr (PK::FF && ((TAB && VAMP_WIDE_NODES) || FFG)) {
        unsigned long long wm = __ballot(my_wide);
        if constexpr (FFG) wm |= (__ballot(my_tiny) ? 1ull << 16 : 0ull) | (__ballot(my_reach) ? 1ull << 17 : 0ull);
        if (writer && lane == 0) L.theta[WIDE_SLOT] = __longlong_as_double((long long)wm);
    }
    if (R.sample_sd && lane == PK::KCAP && writer) {      // one otherwise idle lane: sd ~ U(0,1), vpfits.py:39
        lp = uniform_logp(L.theta[R.D - 1], 0.0, 1.0, 0.0);
    }
    lp = wave_sum<PK::LPW>(lp);
    if constexpr (PK::SPLIT) {
        if (writer && lane == 0) L.theta[LP_SLOT] = lp;
    }
    group_barrier<PK>();
    if constexpr (PK::SPLIT) lp = L.theta[LP_SLOT];
    double (*dt)[vamp::DTAB_N];
    if constexpr (PK::DTAB_IN_TABLES && TAB)
        dt = reinterpret_cast<double (*)[vamp::DTAB_N]>(tab + PK::KCAP * vamp::TAB_LINE - PK::KCAP * vamp::DTAB_N);
    else if constexpr (TAB32)
        dt = reinterpret_cast<double (*)[vamp::DTAB_N]>(tab + TAB32_DOUBLES);     // behind the float rows
    else
        dt = L.dtab;
#ifdef VAMP_SKIP_DTAB     // timing-only builds (tools/variants.py)
    if (false) {
#else
    if (MODE != VAMP_GAUSS3 && (!want_f32 || TAB32 || DT32)) {      // (DT32: an fp32 blend builds its rows from L.dtab)
#endif
        constexpr int STEP = PK::SPLIT ? PK::THREADS : PK::LPW;
        for (int e = PK::SPLIT ? 64 * part + lane : lane; e < K * vamp::DTAB_N; e += STEP) {
            const int k = e / vamp::DTAB_N, n = e % vamp::DTAB_N;
            dt[k][n] = vamp::core_dtab_entry(n, L.line[k].y);
        }
    }
    group_barrier<PK>();
#ifdef VAMP_SKIP_TAB      // timing-only builds (tools/variants.py)
    if constexpr (false) {
#else
    if constexpr (TAB) {
#endif
        // one (line, interval) pair per thread: 16 lines x 16 intervals = the 256 threads of a split
        // group; a single wavefront takes its walker's pairs 64 at a time
        constexpr int TSTEP = PK::SPLIT ? PK::THREADS : PK::LPW;
        if constexpr (PK::DTAB_IN_TABLES) {
            // the near-axis tables occupy the tail of the Taylor tables: every thread reads what its row's centre
            // needs, and only when all have done so are the rows written (one (line, interval) pair per thread)
            static_assert(KMAX * vamp::TAB_NI <= PK::THREADS && PK::KCAP * vamp::DTAB_N <= PK::KCAP * vamp::TAB_LINE, "one row per thread");
            const int e = 64 * part + lane, k = e / vamp::TAB_NI, i = e % vamp::TAB_NI;
            double c0r = 0.0, c0i = 0.0;
            if (e < K * vamp::TAB_NI) vamp::core_centre(i, L.line[k].y, dt[k], L.line[k].pole, L.line[k].hy, c0r, c0i);
            group_barrier<PK>();
            if (e < K * vamp::TAB_NI) vamp::taylor_table_row_from_centre(i, L.line[k].y, c0r, c0i, tab + k * vamp::TAB_LINE + i * vamp::TAB_NT);
        } else {
            for (int e = PK::SPLIT ? 64 * part + lane : lane; e < K * vamp::TAB_NI; e += TSTEP) {
                const int k = e / vamp::TAB_NI, i = e % vamp::TAB_NI;
                vamp::taylor_table_row(i, L.line[k].y, dt[k], L.line[k].pole, L.line[k].hy,
                                       tab + k * vamp::TAB_LINE + i * vamp::TAB_NT);
            }
        }
        group_barrier<PK>();
    }
    if constexpr (TAB32) {
        // fp32 rows: one (line, interval) pair per thread, centre values in double from the near-axis tables
        static_assert(PK::SPLIT && KMAX * vamp::TAB_NI <= PK::THREADS, "one row per thread");
        const int e = 64 * part + lane, k = e / vamp::TAB_NI, i = e % vamp::TAB_NI;
        if (e < K * vamp::TAB_NI)
            vamp::taylor_table_row32(i, L.line[k].y, dt[k], L.line[k].pole, L.line[k].hy,
                                     reinterpret_cast<float*>(tab) + k * vamp::TAB32_LINE + i * vamp::TAB32_NT);
        group_barrier<PK>();
    }
    return lp;
}

// sqrt(pi) H for the TPIX pixels a lane holds, with ONE branch for the whole wavefront.
// Consecutive lanes hold consecutive pixels, so |z| is monotone along the wave on either side of
// the line centre; the wave takes the deepest branch any of its pixels needs (a deeper J-fraction
// is valid wherever a shallower one is).  Only waves that straddle |z|^2 = 64 diverge.
#ifndef VAMP_TPIX
#define VAMP_TPIX 4
#endif
constexpr int TPIX = VAMP_TPIX;      // pixels per lane per iteration in full tiles (the tail of a
                                     // region runs one pixel per lane, so short regions waste nothing)
#ifndef VAMP_SMALL_TPIX
#define VAMP_SMALL_TPIX 4
#endif
// several walkers per wavefront: pixels per lane and iteration (each near-axis evaluation in flight holds ~40 VGPRs)
template <class PK>
constexpr int pixels_per_lane() { return PK::SUBS > 1 ? VAMP_SMALL_TPIX : TPIX; }

template <int M, int T>
__device__ __forceinline__ void tile_jfrac(const double (&X)[T], const double (&r2)[T], double y, double (&H)[T]) {
    int t = 0;
#pragma unroll
    for (; t + 1 < T; t += 2) vamp::voigt_jfrac_x2<M>(X[t], X[t + 1], y, r2[t], r2[t + 1], H[t], H[t + 1]);
    if (t < T) H[t] = vamp::voigt_jfrac<M>(X[t], y, r2[t]);
}

// sqrt(pi) H from the line's Taylor table, 0 <= x < 8: TAB_NT / 2 16-byte LDS reads + TAB_NT - 1 fused multiply-adds
__device__ __forceinline__ double table_eval(const double* tab, double x) {
    // interval i = floor(2 x) as round-to-nearest of 2 (x - 1/4): adding 2^52 + 2^51 leaves the integer in the
    // low word of the sum (no conversions), and on a boundary either neighbour is right (|d| = 1/4 in both)
    constexpr double MAGIC = 6755399441055744.0;
    const double xs = x - 0.5 * vamp::CORE_H;
    const double t = fma(xs, 2.0, MAGIC);
    const int i = __double2loint(t);
    const double d = fma(t - MAGIC, -vamp::CORE_H, xs);
    static_assert(vamp::CORE_H == 0.5, "interval width 1/2");
    static_assert(vamp::TAB_NT % 2 == 0, "coefficient pairs below");
    constexpr int NP = vamp::TAB_NT / 2;
    // (v_mad_u32_u24: the 32-bit integer multiply runs at a quarter of the rate)
    const double2* a = reinterpret_cast<const double2*>(reinterpret_cast<const char*>(tab) + __mul24(i, vamp::TAB_NT * (int)sizeof(double)));
    double2 c[NP];
#pragma unroll
    for (int n = NP - 1; n >= 0; --n) c[n] = a[n];
    double r = fma(c[NP - 1].y, d, c[NP - 1].x);
#pragma unroll
    for (int n = NP - 2; n >= 0; --n) {
        r = fma(r, d, c[n].y);
        r = fma(r, d, c[n].x);
    }
    return r;
}
// table_eval for two pixels of a lane: both rows are requested before either Horner chain starts, and the chains go
// step by step side by side, so that one wait serves both rows and each multiply-add's latency is covered by the
// other chain's.  Per pixel the operations and their order are table_eval's.
__device__ __forceinline__ void table_eval2(const double* tab, double x0, double x1, double& r0, double& r1) {
    constexpr double MAGIC = 6755399441055744.0;
    constexpr int NP = vamp::TAB_NT / 2;
    const double x[2] = {x0, x1};
    double d[2], r[2];
    double2 c[2][NP];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double xs = x[p] - 0.5 * vamp::CORE_H;
        const double t = fma(xs, 2.0, MAGIC);
        const int i = __double2loint(t);
        d[p] = fma(t - MAGIC, -vamp::CORE_H, xs);
        const double2* a = reinterpret_cast<const double2*>(reinterpret_cast<const char*>(tab) + __mul24(i, vamp::TAB_NT * (int)sizeof(double)));
#pragma unroll
        for (int n = NP - 1; n >= 0; --n) c[p][n] = a[n];
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) r[p] = fma(c[p][NP - 1].y, d[p], c[p][NP - 1].x);
#pragma unroll
    for (int n = NP - 2; n >= 0; --n) {
#pragma unroll
        for (int p = 0; p < 2; ++p) r[p] = fma(r[p], d[p], c[p][n].y);
#pragma unroll
        for (int p = 0; p < 2; ++p) r[p] = fma(r[p], d[p], c[p][n].x);
    }
    r0 = r[0], r1 = r[1];
}
// the table for the T pixels of a lane as the library was built (VAMP_TAB_PAIR)
template <int T>
__device__ __forceinline__ void table_eval_tile(const double* tab, const double (&X)[T], double (&H)[T]) {
    int t = 0;
#if VAMP_TAB_PAIR
#pragma unroll
    for (; t + 1 < T; t += 2) table_eval2(tab, X[t], X[t + 1], H[t], H[t + 1]);
#endif
#pragma unroll
    for (; t < T; ++t) H[t] = table_eval(tab, X[t]);
}

// true when pred holds on some active lane of this lane's walker group (LPW lanes; the wavefront when LPW = 64).  The
// branches of the tile evaluators below are voted per group, not per wavefront: every branch is accurate but not
// bit-identical to the others, and a vote over the wavefront would make a walker's value depend on the walkers that
// share its wavefront in the packed shapes -- a point would get other bits in a batch than alone (vamp_lnprob of one
// point, the MAP search's candidates).
template <int LPW>
__device__ __forceinline__ bool group_any(bool pred) {
    if constexpr (LPW == 64) return __any(pred);
    else {
        const int first = (int)(threadIdx.x & 63) & ~(LPW - 1);
        return ((__ballot(pred) >> first) & ((1ull << LPW) - 1ull)) != 0ull;
    }
}

// `tab` (TAB = true): the line's Taylor table replaces the near-axis rule for |z|^2 < 64
template <int T, bool TAB = false, int LPW = 64>
__device__ __forceinline__ void tile_voigt(const LineRec& ln, const double* dtab, const double (&Xin)[T], double (&H)[T],
                                           const double* tab = nullptr, const double* ec = nullptr) {
    // ec: the exp constants in LDS (tile kernels with the far-field table) or null (literals)
    auto gauss_tail = [ec](double xx) { return ec ? vamp::exp_neg_sq_tab(xx, ec) : vamp::exp_neg_sq(xx); };
    const double y = ln.y;
    const double y2 = y * y;
    // narrow line: |z| spans many units (possibly decades) inside one tile, and a lane promoted to a
    // deep fraction would overflow |Q|^2 ~ |z|^(4m).  Such lines carry xcap = X_FAR (else +inf):
    // lanes beyond it are clamped into the range of the fractions here and get the closed far form
    // below.  One v_min per evaluation; the patch is a wave-uniform branch.
    const double xcap = ln.xcap;
    double X[T];
    if (xcap < __builtin_huge_val()) {           // (wave-uniform: four v_min less per line and tile for ordinary lines)
#pragma unroll
        for (int t = 0; t < T; ++t) X[t] = fmin(Xin[t], xcap);
    } else {
#pragma unroll
        for (int t = 0; t < T; ++t) X[t] = Xin[t];
    }
    double r2[T];
    double lo;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        r2[t] = fma(X[t], X[t], y2);
        lo = t ? fmin(lo, r2[t]) : r2[0];
    }
#ifdef VAMP_FORCE_TIER   // timing-only builds (tools/tier_cost.py): every tile takes one branch
    {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const double xx = X[t] < 6.4 ? X[t] : 6.4;
            if (VAMP_FORCE_TIER == 0) H[t] = vamp::voigt_core(xx, y, dtab, ln.pole, ln.hy);
            else if (VAMP_FORCE_TIER == 1) H[t] = vamp::voigt_jfrac<6>(X[t], y, r2[t]);
            else if (VAMP_FORCE_TIER == 2) H[t] = vamp::voigt_jfrac<4>(X[t], y, r2[t]);
            else if (VAMP_FORCE_TIER == 3) H[t] = vamp::voigt_jfrac<3>(X[t], y, r2[t]);
            else if (VAMP_FORCE_TIER == 4) H[t] = vamp::voigt_jfrac<2>(X[t], y, r2[t]);
            else if (VAMP_FORCE_TIER == 5) H[t] = vamp::voigt_far(X[t], y, r2[t]);
            else H[t] = X[t] * y;
        }
        return;
    }
#endif
    if (group_any<LPW>(lo < vamp::R2_M3)) {
        if (group_any<LPW>(lo < vamp::R2_M4)) {
            if (group_any<LPW>(lo < vamp::R2_CORE)) {
#if VAMP_CORE_FASTPATH
                // every pixel of the wavefront inside the zone (the usual case where a line is near): straight-line code,
                // T independent chains with all their LDS reads in flight together.  Behind per-pixel branches (below:
                // a wavefront that straddles |z| = 8) the T evaluations run one after the other, each waiting for its own
                // reads -- what a latency-bound small ensemble spends most of its sweep on
                double hi = r2[0];
#pragma unroll
                for (int t = 1; t < T; ++t) hi = fmax(hi, r2[t]);
                if (!group_any<LPW>(!(hi < vamp::R2_CORE))) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        if constexpr (TAB) H[t] = table_eval(tab, X[t]);
                        else H[t] = vamp::voigt_core(X[t], y, dtab, ln.pole, ln.hy);
                    }
                    return;          // (inside |z| < 8 no pixel is beyond xcap = X_FAR)
                }
#endif
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    if (r2[t] < vamp::R2_CORE) {
                        if constexpr (TAB) H[t] = table_eval(tab, X[t]);
                        else H[t] = vamp::voigt_core(X[t], y, dtab, ln.pole, ln.hy);
                    } else {
                        H[t] = vamp::voigt_jfrac<6>(X[t], y, r2[t]);
                    }
                }
                if (y < vamp::Y_TINY) {
#pragma unroll
                    for (int t = 0; t < T; ++t)
                        if (!(r2[t] < vamp::R2_CORE)) H[t] += vamp::SQRT_PI * gauss_tail(X[t]);
                }
            } else {
                tile_jfrac<6, T>(X, r2, y, H);
                if (y < vamp::Y_TINY) {
#pragma unroll
                    for (int t = 0; t < T; ++t) H[t] += vamp::SQRT_PI * gauss_tail(X[t]);
                }
            }
        } else {
            tile_jfrac<4, T>(X, r2, y, H);
        }
    } else if (group_any<LPW>(lo < vamp::R2_M2)) {
        tile_jfrac<3, T>(X, r2, y, H);
    } else if (group_any<LPW>(lo < vamp::R2_M1)) {
        tile_jfrac<2, T>(X, r2, y, H);
    } else {
#pragma unroll
        for (int t = 0; t < T; ++t) H[t] = vamp::voigt_far(Xin[t], y, fma(Xin[t], Xin[t], y2));
    }
    // (for |z|^2 >= 196 the missing e^{-x^2} is < 1e-85: no tiny-y correction needed there)
    if (xcap < __builtin_huge_val()) {
#pragma unroll
        for (int t = 0; t < T; ++t)
            if (Xin[t] > vamp::X_FAR) H[t] = vamp::voigt_far(Xin[t], y, fma(Xin[t], Xin[t], y2));
    }
}

// chi^2 sweep, fp64 pixel arithmetic.  Returns sum over the walker's pixels of ((f-m) w)^2.
// Full tiles: a lane holds TPIX pixels (i, i+LPW, ...) per iteration -- TPIX independent dependency
// chains and one LDS read of the line record per TPIX evaluations; the remaining pixels of the
// region run one per lane.
template <int MODE, class PK, int T, bool TAB = false>
__device__ __forceinline__ void sweep_range(const RegionDev& R, const typename PK::Lds& L, const double* __restrict__ x,
                                            const double* __restrict__ f, const double* __restrict__ wt, int lane,
                                            int base0, int base1, int stride, double& chi, const double* tab = nullptr) {
    const int K = R.K, P = R.P;
    constexpr bool gauss = (MODE == VAMP_GAUSS3);
    constexpr int LPW = PK::LPW;
    for (int base = base0; base < base1; base += stride) {
        double xi[T], tau[T];
        int idx[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int i = base + LPW * t + lane;
            idx[t] = i < P ? i : P - 1;          // tail lanes recompute the last pixel and drop it
            xi[t] = x[idx[t]];
            tau[t] = 0.0;
        }
#if VAMP_SR_EARLY
        // flux and weights requested now, used after the evaluations: their L2 round trip overlaps the
        // arithmetic instead of following it (the compiler sinks loads to their use)
        double fi[T], wi[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            fi[t] = f[idx[t]];
            wi[t] = wt[idx[t]];
        }
        __builtin_amdgcn_sched_barrier(0);
#endif
        VAMP_STAMP_AFTER(31, xi[0]);
        if constexpr (gauss) {
            for (int k = 0; k < K; ++k) {
                const double c = L.line[k].c, s = L.line[k].s, a = L.line[k].amp;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const double u = (xi[t] - c) * s;
                    tau[t] += a * exp(-0.5 * (u * u));
                }
            }
        } else {
            for (int k = 0; k < K; ++k) {
                const LineRec ln = L.line[k];
                double X[T], H[T];
#pragma unroll
                for (int t = 0; t < T; ++t) X[t] = fabs(xi[t] - ln.c) * ln.s;
                tile_voigt<T, TAB, PK::LPW>(ln, dtab_row<PK>(L, k), X, H, TAB ? tab + k * vamp::TAB_LINE : nullptr);
#pragma unroll
                for (int t = 0; t < T; ++t) tau[t] = fma(ln.amp, H[t], tau[t]);
            }
        }
        VAMP_STAMP_AFTER(32, tau[0]);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const double m = vamp::exp_taylor(-tau[t]);
#if VAMP_SR_EARLY
            const double r = (fi[t] - m) * wi[t];
#else
            const double r = (f[idx[t]] - m) * wt[idx[t]];
#endif
            const bool live = (base + LPW * t + lane) < P;
            chi += live ? r * r : 0.0;
        }
        VAMP_STAMP_AFTER(33, chi);
    }
}

// ---- far-field aggregation ----------------------------------------------------------------
// Seen from a tile of 256 consecutive pixels, a line whose centre lies >= FF_DIST half-widths
// beyond the tile's edge contributes an optical depth that is analytic across the tile with its
// nearest singularity (the line centre) that far away: a degree-15 Chebyshev interpolant
// reproduces it to 6e-13 relative (singularity at (FF_DIST + 1) half-widths from the tile centre:
// Bernstein ellipse parameter 3 + sqrt(8) = 5.8 for FF_DIST = 2, and 5.8^-16 = 6e-13; FF_DIST = 4: 9.9^-16 = 1.2e-16).  Polynomials add, so ALL far lines of the tile share one interpolant:
//   1. the (node, far line) pairs -- 16 nodes x up to 16 lines -- are spread over the 64 lanes
//      (lane = 16 * (line slot) + node) and evaluated with the same Voigt code, 4 lines per pass;
//   2. node values are summed over lines (two xor shuffles) and turned by ONE 56 x 16 matrix held in
//      LDS (one row per lane, tools/gen_ff_matrix.py) into four local power series, one per quarter
//      of the tile -- a lane holds one pixel of each quarter -- with 14 coefficients each: seen from
//      a quarter's centre the far lines are >= 9 quarter half-widths away, the coefficients fall
//      like 9^-j and the terms beyond u^13 are < 3e-11 of the value (of a wing that is itself a small part
//      of the optical depth there);
//   3. every pixel of the tile runs Horner's rule on its quarter's series: 13 fused multiply-adds
//      (Clenshaw's recurrence on the tile's Chebyshev coefficients cost 30) instead of ~27
//      instructions per far line.
// On the headline workload ~90 % of the (pixel, line) evaluations are far: 64 wave-evaluations
// per tile shrink to ~6 direct ones + ~4 at the nodes.
constexpr int FF_EXP = FF_MAT + FF_NODES;     // constants of the exp kernel (vamp::exp_taylor_tab), 16-byte aligned
constexpr int FF_TABLE = FF_EXP + vamp::EXP_TAB_N;   // the matrix [n/2][lane][n%2], the node abscissae, the exp constants
__device__ const double EXP_TAB[vamp::EXP_TAB_N] = VAMP_EXP_TAB_INIT;

// fp32 contexts: the 32 x 8 matrix of the 8-node interpolant and its node abscissae, as floats (1 KB instead of 7.4)
constexpr int FF32_TABLE = FF32_MAT + FF32_NODES;
template <bool F32>
constexpr int ff_table_doubles() { return F32 ? (FF32_TABLE + 1) / 2 : FF_TABLE; }
// every thread of the workgroup copies its share; call before any thread can leave the kernel
template <bool F32>
__device__ __forceinline__ void ff_fill_table(double* dct) {
    if constexpr (F32) {
        float* d32 = reinterpret_cast<float*>(dct);
        for (int e = threadIdx.x; e < FF32_TABLE; e += blockDim.x) d32[e] = FF32_M[e];
    } else {
        for (int e = threadIdx.x; e < FF_TABLE; e += blockDim.x) dct[e] = e < FF_EXP ? FF_M[e] : EXP_TAB[e - FF_EXP];
    }
    __syncthreads();
}

// sqrt(pi) H at one point per slot for different lines per lane (x[t], y[t]), two slots at a time;
// every point has |z|^2 >= 64.  One branch for the wavefront per slot PAIR, the deepest any of its
// 128 points needs, and one reciprocal per pair.  (The far list is ordered deep lines first, so the
// second pair usually runs the cheapest fraction.)
template <int M>
__device__ __forceinline__ void ff_frac2(const double (&X)[2], const double (&y)[2], const double (&r2)[2], double (&H)[2]) {
    double n[2], d[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) vamp::voigt_jfrac_nd<M>(X[t], y[t], r2[t], n[t], d[t]);
    const double ra = vamp::rcp_nr(d[0] * d[1]);
    H[0] = n[0] * (ra * d[1]);
    H[1] = n[1] * (ra * d[0]);
}

// GUARD = false: staging has established for this walker (ff_guard_bits) that no line reaches X > X_FAR at a node of the
// region and none has y < Y_TINY -- the clamp is the identity and neither patch can fire, so they are not compiled: the
// same bits from about six vector instructions fewer per call.
template <bool GUARD = true>
__device__ __forceinline__ void ff_eval2(const double (&Xin)[2], const double (&y)[2], double (&H)[2], const double* ec) {
    // The clamp bounds the fractions' argument in BOTH coordinates: the two slots share one reciprocal of d0 d1 (ff_frac2),
    // so a denominator that overflows -- X or y beyond ~1e38; y = L sqrt(ln 2) / G is unbounded where L is the region's
    // and G -> 0 (NBZ3) -- would turn its PARTNER's value into NaN, and the partner is not patched.  A walker without the
    // reach bit has X <= X_FAR and y = (L / 2) s <= 1.2 X_FAR (L <= fwhm_max): nothing to bound in the unguarded copy.
    double X[2], yc[2], r2[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        X[t] = GUARD ? fmin(Xin[t], vamp::X_FAR) : Xin[t];       // lanes hold different lines: guard the promotion
        yc[t] = GUARD ? fmin(y[t], vamp::X_FAR) : y[t];
        r2[t] = fma(X[t], X[t], yc[t] * yc[t]);
    }
    const double lo = fmin(r2[0], r2[1]);
    // the fractions' ranges for NODE values: 4e-13 / 2e-13 / 9e-13 of the value at the lower ends (the m-level fraction is
    // the 2m-point Gauss-Hermite rule of w's integral; the pixel evaluator's own ranges, R2_M4 / M3 / M2 = 196 / 625 / 1e4,
    // hold 2e-15) -- the series these values feed reproduce a wing to 3e-11 of its value
    constexpr double N_M4 = VAMP_FF_R2_M4, N_M3 = VAMP_FF_R2_M3, N_M2 = VAMP_FF_R2_M2;
    if (__any(lo < N_M3)) {
        if (__any(lo < N_M4)) ff_frac2<6>(X, yc, r2, H);
        else ff_frac2<4>(X, yc, r2, H);
    } else if (__any(lo < N_M2)) {
        ff_frac2<3>(X, yc, r2, H);
    } else {
        ff_frac2<2>(X, yc, r2, H);              // valid (more than accurate) beyond 1e8 too, up to X_FAR
    }
    if constexpr (!GUARD) return;
    const double hi = fmax(fmax(Xin[0], Xin[1]), fmax(y[0], y[1])), ymin = fmin(y[0], y[1]);
    if (__any(hi > vamp::X_FAR)) {              // either coordinate beyond X_FAR: |z|^2 >= R2_M1, voigt_far's range
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (Xin[t] > vamp::X_FAR || y[t] > vamp::X_FAR) H[t] = vamp::voigt_far(Xin[t], y[t], fma(Xin[t], Xin[t], y[t] * y[t]));
    }
    if (__any(ymin < vamp::Y_TINY)) {           // the fractions miss e^{-x^2}; it matters for y < ~1e-11 near |z| = 8
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (y[t] < vamp::Y_TINY) H[t] += vamp::SQRT_PI * vamp::exp_neg_sq_tab(X[t], ec);
    }
}

// far-field steps shared by the fp64 and the fp32 sweep.  All wave-uniform in control flow.
// (a) classification of all lines against the wavefront's next FF_BATCH tiles (base, base + stride, ...) at once: lane
//     16 j + k holds line k and tile j.  far = centre >= FF_DIST half-widths beyond the tile's edge and the whole
//     tile outside |z|^2 < 64 of that line (fp32 contexts: outside the line's Gaussian core, VAMP_F32_FAR_CORE); far
//     lines that reach into |z|^2 < 625 at the tile's edge need the deep fractions and are listed first.  WIDE: near
//     lines far wider than the tile (`wide_all`), and lines FF_DIST half-widths away whose |z| < 8 zone still reaches
//     into the tile while their Gaussian core does not (VAMP_MID_NODES), go to the wide list.
//     Returns the masks of the four tiles, 16 bits each (tile j in bits 16 j ..), and leaves the compacted lists in
//     Sx.farlist[j] / Sx.widelist[j]; a tile at or past base1 classifies the first tile again and is never consumed.
//     A pure function of (line record, tile edges): it used to run once per tile on 16 of the 64 lanes.
__device__ __forceinline__ unsigned ff_tile_field(unsigned long long batchmask, int lane) {   // the 16 bits of this lane's tile
    const unsigned h = (lane & 32) ? (unsigned)(batchmask >> 32) : (unsigned)batchmask;
    return (h >> (lane & 16)) & 0xffffu;
}
//     ZONE (fp64 loop with the lines' Taylor tables): a third mask, bit set = the whole tile lies inside the line's table
//     zone (vamp::ff_tile_in_zone); the near-line loop consults it for its near lines and skips tile_voigt's votes.
template <bool WIDE, bool F32, bool ZONE = false, class LDS>
__device__ __forceinline__ void ff_classify_batch(const LDS& L, TileScratch& Sx, const double2* __restrict__ geo, int K, int lane_, int base,
                                                  int base1, int stride, unsigned wide_all,
                                                  unsigned long long& farmasks, unsigned long long& widemasks, unsigned long long& zonemasks) {
    // everything a lane derives from its index is derived here, once per batch, from an opaque copy: hoisted out of
    // the tile loop these values would sit in registers the loop does not have (and come back from scratch)
    int lane = lane_;
    asm volatile("" : "+v"(lane));
    const int j = lane >> 4, k = lane & (KMAX - 1);
    const unsigned below = (1u << k) - 1u;
    int bj = base + j * stride;
    bj = bj < base1 ? bj : base;
    const double2 g = geo[bj >> 8];       // (mid, half) of "its" tile: one load instead of two abscissae and their arithmetic
    const double mid = g.x, half = fabs(g.y);
    // centre and zone half-widths of "its" line: four LDS reads per batch, all issued together (no short-circuit
    // evaluation below: the predicates are bit operations on compare results, the pass has no branches but the writes)
    const LineRec& me = *reinterpret_cast<const LineRec*>(reinterpret_cast<const char*>(L.line) +
                                                          __umul24((unsigned)(k < K ? k : 0), (unsigned)sizeof(LineRec)));
    const double my_c = me.c, my_w8 = me.w8, my_w25 = me.w25, my_wmid = me.wmid;
    const double dist = fabs(mid - my_c) - half;
    const bool my_beyond = (k < K) & (dist >= FF_DIST * half);
    const bool my_far = my_beyond & (dist >= ((F32 && VAMP_F32_FAR_CORE) ? my_wmid : my_w8));
    const bool my_deep = my_far & (dist < my_w25);
    farmasks = __ballot(my_far);
    // far list of a tile: its deep lines in line order, then the other far lines in line order.  The place of line k is
    // the number of list members ahead of it (deep is a subset of far)
    const unsigned far16 = ff_tile_field(farmasks, lane), deep16 = ff_tile_field(__ballot(my_deep), lane);
    const unsigned ahead = my_deep ? (deep16 & below) : (deep16 | (far16 & below));
    if (my_far) Sx.farlist[j][__builtin_popcount(ahead)] = (unsigned char)k;
    // INVARIANT the tile loop relies on (sweep_range_ff, the mark of a tile done from its moments): no line is ever listed
    // as far AND wide for one tile -- my_wide carries `& !my_far`, and widemasks is zero without WIDE -- so a field with
    // bits set in BOTH masks cannot come from here.  Whoever changes that must give the mark another place.
    widemasks = 0ull;
    if constexpr (WIDE) {
        const bool my_wide = ((((wide_all >> k) & 1u) != 0u) | (VAMP_MID_NODES && (my_beyond & (dist >= my_wmid)))) & !my_far;
        widemasks = __ballot(my_wide);
        if (my_wide) Sx.widelist[j][__builtin_popcount(ff_tile_field(widemasks, lane) & below)] = (unsigned char)k;
    }
    zonemasks = 0ull;
    if constexpr (ZONE) zonemasks = __ballot(vamp::ff_tile_in_zone(my_c, me.s, me.y, mid, half));
    __builtin_amdgcn_wave_barrier();      // (the lists are in LDS; their readers follow in the tiles' iterations)
}
// node sums (lanes 0..15 hold them) -> the four local power series of the tile: lane l = 14 q + j < 56 owns
// coefficient j of quarter q, a = sum_n M[l][n] f_n, stored in the pixel arithmetic type
template <class real>
__device__ __forceinline__ void ff_series(TileScratch& Sx, const double* __restrict__ dct, int lane, double fs) {
    if (lane < FF_NODES) Sx.coef[lane] = fs;
    __builtin_amdgcn_wave_barrier();
    const double2* mrow = reinterpret_cast<const double2*>(dct) + (lane < FF_ROWS ? lane : FF_ROWS - 1);
    const double2* fv = reinterpret_cast<const double2*>(Sx.coef);
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int n2 = 0; n2 < FF_NODES / 2; ++n2) {
        const double2 m = mrow[n2 * FF_ROWS], f2 = fv[n2];
        a0 = fma(m.x, f2.x, a0);
        a1 = fma(m.y, f2.y, a1);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < FF_ROWS) reinterpret_cast<real*>(Sx.coef)[lane] = (real)(a0 + a1);
    __builtin_amdgcn_wave_barrier();
}
// (b) optical depth of the far lines at the tile's Chebyshev nodes -> the tile's local power series in Sx.coef
//     (fp32 contexts: ff32_coefficients below, 8 nodes)
//     ff_node_sums: the node stage alone -- every lane ends with the sum of its node (lane & 15)
template <class LDS, bool GUARD = true>
__device__ __forceinline__ double ff_node_sums(const LDS& L, const unsigned char* farlist, const double* __restrict__ dct,
                                               int lane_, int nfar, double mid, double half, double fs_wide = 0.0) {
    int lane = lane_;
    asm volatile("" : "+v"(lane));      // (as in ff_classify_batch: node and group are derived per tile, not kept in registers)
    const int node = lane & (FF_NODES - 1), grp = lane >> 4;
    const double tnode = dct[FF_MAT + node];                       // cos(pi (node + 1/2) / 16)
    __builtin_amdgcn_wave_barrier();
    // 1. lane = (slot group, node), four lines per lane (line q = 4 t + group of the compacted far list)
    const double xnode = fma(half, tnode, mid);
    double Xn[4], yn[4], an[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int q = 4 * t + grp;
        const unsigned kf = nfar > 0 ? farlist[q < nfar ? q : nfar - 1] : 0u;
        const LineRec& ln = *reinterpret_cast<const LineRec*>(reinterpret_cast<const char*>(L.line) + __umul24(kf, (unsigned)sizeof(LineRec)));
        Xn[t] = fabs(xnode - ln.c) * ln.s;
        yn[t] = ln.y;
        an[t] = q < nfar ? ln.amp : 0.0;
    }
    double fs = 0.0;
    if (nfar > 0) {
        const double Xa[2] = {Xn[0], Xn[1]}, ya[2] = {yn[0], yn[1]};
        double Ha[2];
        ff_eval2<GUARD>(Xa, ya, Ha, dct + FF_EXP);
        fs = fma(an[0], Ha[0], an[1] * Ha[1]);
    }
    if (nfar > 8) {                               // list entries 8..15 (slots 2, 3)
        const double Xb[2] = {Xn[2], Xn[3]}, yb[2] = {yn[2], yn[3]};
        double Hb[2];
        ff_eval2<GUARD>(Xb, yb, Hb, dct + FF_EXP);
        fs += fma(an[2], Hb[0], an[3] * Hb[1]);
    }
    fs += fs_wide;
    // the sums of the four slot groups: the partners' addresses from the opaque lane index, per tile -- __shfl_xor keeps
    // them in two registers for the whole loop, which k_lnprob's loop does not have (it reloaded them from scratch)
    fs += __hiloint2double(__builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, __double2hiint(fs)),
                           __builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, __double2loint(fs)));
    fs += __hiloint2double(__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __double2hiint(fs)),
                           __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __double2loint(fs)));
    return fs;
}
template <class LDS, bool GUARD = true>
__device__ __forceinline__ void ff_coefficients(const LDS& L, TileScratch& Sx, const unsigned char* farlist, const double* __restrict__ dct,
                                                int lane, int nfar, double mid, double half, double fs_wide = 0.0) {
    ff_series<double>(Sx, dct, lane, ff_node_sums<LDS, GUARD>(L, farlist, dct, lane, nfar, mid, half, fs_wide));
}
// (d) chi^2 of a tile whose optical depth is the interpolant alone, from the context's data moments `mt` of the tile
//     (ff_moments.hpp) instead of its pixels.  `a`: the absorption 1 - e^{-tau} at the lane's node, from the node sums.
//     ff_series turns it into the four series b_q of the absorption; lane 14 q + j < 56 then adds its share
//     b_q[j] (sum_l b_q[l] Q_q[j + l] + 2 S_q[j]) of C0 + 2 b.S + b'Qb and lane 56 adds C0.  Written on (f - 1, a)
//     rather than (f, m) the form cancels mildly where the model fits; how mildly is the guard's business (the caller's).
__device__ __forceinline__ void ff_moment_chi(TileScratch& Sx, const double* __restrict__ dct, const double* __restrict__ mt, int lane,
                                              double a, double& chi) {
    const int row = lane < FF_ROWS ? lane : FF_ROWS - 1;
    const int q = row / (FF_DEG + 1), j = row - q * (FF_DEG + 1);
    ff_series<double>(Sx, dct, lane, a);
    // (requested after the transform, whose own loads fill the registers: ahead of it the window costs the loop spills)
    const double* Qw = mt + q * vamp::FFM_QROW + j;          // Q_q[j .. j + 13]: a contiguous window per lane
    double Qv[FF_DEG + 1];
#pragma unroll
    for (int l = 0; l <= FF_DEG; ++l) Qv[l] = Qw[l];
    const double Sv = mt[vamp::FFM_S + row], c0 = mt[vamp::FFM_C0];
    const double* bq = Sx.coef + q * (FF_DEG + 1);
    double acc0 = Sv + Sv, acc1 = 0.0;
#pragma unroll
    for (int l = 0; l <= FF_DEG; l += 2) {
        acc0 = fma(bq[l], Qv[l], acc0);
        acc1 = fma(bq[l + 1], Qv[l + 1], acc1);
    }
    const double term = Sx.coef[row] * (acc0 + acc1);
    chi += lane < FF_ROWS ? term : lane == FF_ROWS ? c0 : 0.0;
    __builtin_amdgcn_wave_barrier();
}
// (d') the same chi^2 from the tile's node record (ff_moments.hpp, VAMP_TILE_MOMENTS == 2): a quadratic form in the node
//     values themselves, C0 + sum_n a_n (2 S'_n + sum_m Q'_nm a_m) -- no transform, no series.  Every row of 16 lanes
//     holds the 16 values; lane 16 g + n takes row n, columns 4 g .. 4 g + 3 of Q' (32 contiguous bytes) and a quarter of
//     2 S'_n (S'_n / 2 four times is 2 S'_n exactly); lane 0 adds C0.  The four a_m of a lane's columns come from the
//     first row's copy in Sx.coef at a row-uniform address.
__device__ __forceinline__ void ff_moment_chi_nodes(TileScratch& Sx, const double* __restrict__ mt, int lane, double a, double c0, double& chi) {
    static_assert(FF_NODES == vamp::FFN_NODES, "the record is laid out for the node stage's 16 nodes");
    if (lane < FF_NODES) Sx.coef[lane] = a;
    const int n = lane & (FF_NODES - 1), g4 = (lane >> 4) * 4;
    const double2* Qr = reinterpret_cast<const double2*>(mt + vamp::FFN_Q + n * FF_NODES + g4);
    const double2 q01 = Qr[0], q23 = Qr[1];
    const double Sv = mt[vamp::FFN_S + n];
    __builtin_amdgcn_wave_barrier();
    const double2* av = reinterpret_cast<const double2*>(Sx.coef + g4);
    const double2 a01 = av[0], a23 = av[1];
    const double acc0 = fma(q01.x, a01.x, 0.5 * Sv), acc1 = q01.y * a01.y;
    const double term = a * (fma(q23.x, a23.x, acc0) + fma(q23.y, a23.y, acc1));
    chi += lane == 0 ? term + c0 : term;
    __builtin_amdgcn_wave_barrier();
}
// the tile's record in the context's table: its size and the places of what the guard reads
constexpr int MOM_TILE = VAMP_TILE_MOMENTS == 2 ? vamp::FFN_TILE : vamp::FFM_TILE;
constexpr int MOM_RC = VAMP_TILE_MOMENTS == 2 ? vamp::FFN_RC : vamp::FFM_RC;
constexpr int MOM_RQ = VAMP_TILE_MOMENTS == 2 ? vamp::FFN_RQ : vamp::FFM_RQ;
// ---- lines far wider than the tile -------------------------------------------------------------------------------
// An ensemble drawn from the priors (widths ~ U(0, fwhm_max): where every find_bic repeat STARTS, vpfits.py:283-297) has
// nothing far: every line is wider than the region, every (line, tile) pair is near and costs four table look-ups per
// lane (profiles/r03_c_headline_robustness.txt: 12.5 ms per swept half-step against 3.4).  But seen from a tile, such a
// line is as smooth as a far one: w is entire, and over a tile whose half-width is at most VAMP_WIDE_MAX = 3/4 in the
// line's own z (G_fwhm >~ 284 px on a unit grid) the degree-15 interpolant through the tile's 16 Chebyshev nodes
// reproduces its optical depth to ~5e-12 of its peak (the first dropped coefficient, 2 e^{-a^2/2} I_8(a^2/2)).  So the roles of "far" and "wide" are exchanged: wide lines are evaluated
// at the NODES -- (node, line) pairs over the lanes as for the far lines, 4 lines per lane, through the line's own
// Taylor table (or the 6-level fraction beyond |z| = 8) -- and join the far lines' node sums before the one transform.
// 16 wide lines: 4 look-ups per lane and tile instead of 64.
template <class LDS>
__device__ __forceinline__ double ff_wide_nodes(const LDS& L, const unsigned char* widelist, const double* __restrict__ dct, const double* tab,
                                                int lane, int nwide, double mid, double half) {
    const int node = lane & (FF_NODES - 1), grp = lane >> 4;
    const double xnode = fma(half, dct[FF_MAT + node], mid);
    double fs = 0.0;
    for (int t = 0; 4 * t < nwide; ++t) {
        const int q = 4 * t + grp;
        const int k = widelist[q < nwide ? q : nwide - 1];
        const LineRec& ln = L.line[k];
        const double X = fabs(xnode - ln.c) * ln.s, r2 = fma(X, X, ln.y * ln.y);
        double H;
        if (r2 < vamp::R2_CORE) {
            H = table_eval(tab + k * vamp::TAB_LINE, X);
        } else {
            H = vamp::voigt_jfrac<6>(X, ln.y, r2);
            if (ln.y < vamp::Y_TINY) H += vamp::SQRT_PI * vamp::exp_neg_sq_tab(X, dct + FF_EXP);
        }
        fs = fma(q < nwide ? ln.amp : 0.0, H, fs);
    }
    return fs;
}
// (c) Horner's rule at the tile's pixels, added to tau (in the pixel arithmetic type).  Register t of a
//     lane is pixel 64 t + lane of the tile: quarter t of an ascending grid, 3 - t of a descending one.
//     u[t]: the pixel's place in its quarter, from the context's table (k_tile_tables).  `up`: the grid ascends.
template <class real, int T>
__device__ __forceinline__ void ff_horner(const TileScratch& Sx, const real (&u)[T], bool up, real (&tau)[T]) {
    static_assert(T == 4, "one pixel per quarter of the tile");
    real acc[T];
    const real* cq[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int q = up ? t : T - 1 - t;
        cq[t] = reinterpret_cast<const real*>(Sx.coef) + q * (FF_DEG + 1);
        acc[t] = cq[t][FF_DEG];
    }
#pragma unroll
    for (int j = FF_DEG - 1; j >= 0; --j) {
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = fma(acc[t], u[t], cq[t][j]);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) tau[t] += acc[t];
    __builtin_amdgcn_wave_barrier();
}

// WIDE: this walker has lines far wider than a tile (ff_wide_nodes).  A copy of the loop of its own, chosen per walker
// by a wave-uniform branch: compiled into the one loop, the wide path cost the converged headline ensemble -- which has no
// such line -- 2.8 % through the loop's register allocation (profiles/r04_e_wide_lines.txt).
// GUARD: some line of this walker needs ff_eval2's clamp or one of its patches (ff_guard_bits); chosen the same way.
// The tile's geometry comes from the context's tables (k_tile_tables): (mid, half) of tile `base` in geo[base >> 8], one
// 16-byte load at a wave-uniform address; the pixels' places in their quarters in ut[], requested after the near lines.
template <int MODE, class PK, bool TAB, bool WIDE = false, bool GUARD = true>
__device__ __forceinline__ void sweep_range_ff(const RegionDev& R, const typename PK::Lds& L, TileScratch& Sx, const double* __restrict__ dct,
                                               const double* __restrict__ x, const double* __restrict__ f,
                                               const double* __restrict__ wt, const double* __restrict__ ut,
                                               const double2* __restrict__ geo, int lane, int base0, int base1, int stride,
                                               double& chi, const double* tab, unsigned long long wide_all = 0ull,
                                               const double* __restrict__ mom = nullptr) {
    constexpr int T = TPIX;
    static_assert(PK::LPW == 64 && PK::KCAP <= 16, "far-field tiles: one walker per wavefront, <= 16 lines");
    const int K = R.K;
#if VAMP_X_PREFETCH
    // the abscissae of a tile are requested one tile ahead: they head every dependency chain of the
    // tile (classification, near lines, far-field series), and an L2 round trip at the top of each of the
    // 16 iterations is paid by all the wavefronts of a workgroup together
    double xn[T];
    if (base0 < base1) {
#pragma unroll
        for (int t = 0; t < T; ++t) xn[t] = x[base0 + 64 * t + lane];
    }
#endif
    // the lines are classified against FF_BATCH tiles at a time, at the top of every FF_BATCH-th tile (ahead of the
    // previous batch's last tiles the pass would hold its loads in registers the loop does not have)
    for (int batch = base0; batch < base1; batch += FF_BATCH * stride) {
    unsigned long long farmasks, widemasks, zonemasks;
    ff_classify_batch<WIDE, false, TAB>(L, Sx, geo, K, lane, batch, base1, stride, (unsigned)wide_all, farmasks, widemasks, zonemasks);
    // Tiles without a near line, in a loop of their own ahead of the others' (compiled into the one loop the branch costs
    // every tile registers the loop does not have): the optical depth is the interpolant alone and the tile's chi^2 a
    // quadratic form in its 16 node values on the tile's node record (ff_moment_chi_nodes; VAMP_TILE_MOMENTS == 1: in its
    // series on moments of the data, ff_moment_chi) -- no pixel is loaded, no transform, no Horner's rule, no
    // exponential per pixel.  The guard (vamp::ff_moments_ok) admits a tile only where the form's cancellation is harmless:
    // first on what the data alone say (amax = 0), then with the largest absorption at the nodes.  A tile it turns away is
    // not marked and is swept pixel by pixel below like any other.  Every decision is wave-uniform.  The mark of a tile
    // that is done: all sixteen bits of its field in BOTH masks -- the classification never lists a line as far and wide --
    // so that the loop below carries no state it did not carry before.
#if VAMP_TILE_MOMENTS && !defined(VAMP_SKIP_FFNODES)
    {
        unsigned long long fm = farmasks, wm = widemasks;
#pragma unroll 1
        for (int j = 0; j < FF_BATCH; ++j, fm >>= KMAX, wm >>= KMAX) {
            const int base = batch + j * stride;
            if (base >= base1) break;
            const unsigned farmask = (unsigned)fm & 0xffffu, widemask = WIDE ? (unsigned)wm & 0xffffu : 0u;
            if ((~(farmask | widemask) & ((1u << K) - 1u)) != 0u) continue;
            const double* mt = mom + (base >> 8) * MOM_TILE;
            const double root_c0 = mt[MOM_RC], root_q0 = mt[MOM_RQ];
            if (!vamp::ff_moments_try(root_c0, root_q0)) continue;
            const double2 tg = geo[base >> 8];
            const double mid = tg.x, half = fabs(tg.y);
            const int nfar = __builtin_popcount(farmask), nwide = __builtin_popcount(widemask);
            const int ln = lane_here();       // (this loop keeps nothing derived from the lane index between its tiles)
            double fs_wide = 0.0;
            if constexpr (WIDE) {
                if (nwide > 0) fs_wide = ff_wide_nodes<typename PK::Lds>(L, Sx.widelist[j], dct, tab, ln, nwide, mid, half);
            }
            const double fs = ff_node_sums<typename PK::Lds, GUARD>(L, Sx.farlist[j], dct, ln, nfar, mid, half, fs_wide);
            int eoff = FF_EXP;
            asm volatile("" : "+s"(eoff));          // (as below: the constants are read here, not kept in registers)
            const double a = -vamp::expm1_taylor_tab(-fs, dct + eoff);
            const double amax = row16_max(fabs(a));      // (every row of 16 lanes holds the 16 nodes)
            if (!__builtin_amdgcn_readfirstlane((int)vamp::ff_moments_ok(root_c0, root_q0, amax))) continue;
#if VAMP_TILE_MOMENTS == 2
            ff_moment_chi_nodes(Sx, mt, ln, a, mt[vamp::FFN_C0], chi);
#else
            ff_moment_chi(Sx, dct, mt, ln, a, chi);
#endif
            const unsigned long long field = 0xffffull << (KMAX * j);
            farmasks |= field;
            widemasks |= field;
        }
    }
#endif
#pragma unroll 1
    for (int j = 0; j < FF_BATCH; ++j, farmasks >>= KMAX, widemasks >>= KMAX, zonemasks >>= KMAX) {
        const int base = batch + j * stride;
        if (base >= base1) break;
        double xi[T], tau[T];
#if VAMP_X_PREFETCH
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xi[t] = xn[t];
            tau[t] = 0.0;
        }
        {
            const int nb = base + stride < base1 ? base + stride : base;     // the last tile re-reads itself
#pragma unroll
            for (int t = 0; t < T; ++t) xn[t] = x[nb + 64 * t + lane];
        }
#else
#if VAMP_TILE_HEAD
        if ((unsigned)farmasks & (unsigned)widemasks & 0xffffu) continue;      // done from its moments: nothing of it is loaded
#endif
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xi[t] = x[base + 64 * t + lane];
            tau[t] = 0.0;
        }
#endif
        if ((unsigned)farmasks & (unsigned)widemasks & 0xffffu) continue;      // done from its moments
        // tile geometry (wave-uniform): the table's half carries the grid's orientation in its sign
        const double2 tg = geo[base >> 8];
        const double mid = tg.x, half = fabs(tg.y);
        const bool up = __double2hiint(tg.y) >= 0;
        // this tile's slice of the batch: masks by scalar bit-field extraction, lists by row
        const unsigned farmask = (unsigned)farmasks & 0xffffu;
        const int nfar = __builtin_popcount(farmask);
        // near lines far wider than the tile join the interpolant (ff_wide_nodes), and so do the lines between "far" and
        // "near" (VAMP_MID_NODES): the centre is FF_DIST half-widths away, the tile still inside |z| < 8 of the line (where
        // the node values cannot be continued fractions) but outside its Gaussian core: as smooth as a far line, evaluated
        // at the nodes through its Taylor table like a wide one.  Needs the lines' Taylor tables
        const unsigned widemask = WIDE ? (unsigned)widemasks & 0xffffu : 0u;
        const int nwide = __builtin_popcount(widemask);
        // near lines: walk the set bits of the complement of the far mask (1-3 of 16 on the headline)
        // (VAMP_SKIP_*: timing-only builds of tools/variants.py -- the phase split in profiles/)
#ifndef VAMP_SKIP_NEAR
        for (unsigned near = ~(farmask | widemask) & ((1u << K) - 1u); near; near &= near - 1u) {
            const int k = __builtin_ctz(near);
            const LineRec ln = L.line[k];
            double X[T], H[T];
#pragma unroll
            for (int t = 0; t < T; ++t) X[t] = fabs(xi[t] - ln.c) * ln.s;
            // the classification has established that every pixel of the tile lies in the line's table zone: the
            // straight-line path tile_voigt would find for itself (same function, same arguments, same bits: inside
            // |z| < 8 no cap binds), without the sixteen instructions and four votes it takes to find it
            if (TAB && (((unsigned)zonemasks >> k) & 1u)) {
                table_eval_tile<T>(tab + k * vamp::TAB_LINE, X, H);
            } else {
                tile_voigt<T, TAB>(ln, dtab_row<PK>(L, k), X, H, TAB ? tab + k * vamp::TAB_LINE : nullptr, dct + FF_EXP);
            }
#pragma unroll
            for (int t = 0; t < T; ++t) tau[t] = fma(ln.amp, H[t], tau[t]);
        }
#endif
        // flux and weights of the tile are requested here, ahead of the far-field series and the
        // exponentials that separate them from their use: left to itself the compiler sinks each
        // load to its use and the wavefront sits through eight L2 round trips per tile
        double fi[T], wi[T];
        if (nfar + nwide > 0) {
            // the pixels' places in their quarters, requested ahead of the node stage that hides the round trip: xi has
            // ended with the near lines, u takes its registers.  (One block from here to Horner's rule: requested in a
            // block of their own the loads are sunk to their use, behind the node stage.)
            double u[T];
#pragma unroll
            for (int t = 0; t < T; ++t) u[t] = ut[base + 64 * t + lane];
#ifndef VAMP_SKIP_FFNODES
            double fs_wide = 0.0;
            if constexpr (WIDE) {
                if (nwide > 0) {
                    fs_wide = ff_wide_nodes<typename PK::Lds>(L, Sx.widelist[j], dct, tab, lane, nwide, mid, half);
                }
            }
            ff_coefficients<typename PK::Lds, GUARD>(L, Sx, Sx.farlist[j], dct, lane, nfar, mid, half, fs_wide);
#endif
#if VAMP_EARLY_LOADS
#pragma unroll
            for (int t = 0; t < T; ++t) {
                fi[t] = f[base + 64 * t + lane];
                wi[t] = wt[base + 64 * t + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
#endif
#ifndef VAMP_SKIP_CLENSHAW
            ff_horner<double, T>(Sx, u, up, tau);
#endif
        } else {
#if VAMP_EARLY_LOADS
#pragma unroll
            for (int t = 0; t < T; ++t) {
                fi[t] = f[base + 64 * t + lane];
                wi[t] = wt[base + 64 * t + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
#endif
        }
        // the exp constants are read from LDS here, per tile: as literals they sit in ~30 SGPRs (or VGPRs) through
        // the whole loop, and the pointers and masks they displace are then reloaded from VGPR lanes in every tile
        int eoff = FF_EXP;
        asm volatile("" : "+s"(eoff));          // (keeps the compiler from hoisting the reads out of the loop)
        const double* ec = dct + eoff;
#pragma unroll
        for (int t = 0; t < T; ++t) {
#if !VAMP_EARLY_LOADS
            fi[t] = f[base + 64 * t + lane];
            wi[t] = wt[base + 64 * t + lane];
#endif
#ifdef VAMP_SKIP_EXP
            const double m = 1.0 - tau[t];
#else
            const double m = vamp::exp_taylor_tab<VAMP_FLUX_EXP_DROP>(-tau[t], ec);
#endif
            const double r = (fi[t] - m) * wi[t];
            chi = fma(r, r, chi);
        }
    }
    }
}

// ---- the node stage of a full batch, line by line (VAMP_NODE_PASS) ----------------------------------------------------
// (The timing-only builds of the phase split, the series form of the moments and the prefetching loop keep sweep_range_ff.)
#if VAMP_NODE_PASS && VAMP_TILE_MOMENTS != 1 && !VAMP_X_PREFETCH && !defined(VAMP_SKIP_NEAR) && !defined(VAMP_SKIP_FFNODES) && \
    !defined(VAMP_SKIP_CLENSHAW) && !defined(VAMP_SKIP_EXP)
#define VAMP_NODE_PASS_ON 1
#else
#define VAMP_NODE_PASS_ON 0
#endif
#if VAMP_NODE_PASS_ON
// ff_classify_batch judges 16 lines against four tiles with lane = 16 j + k.  The node stage of the same four tiles takes
// the transposed mapping, lane = 16 j + node, and a loop over the lines that are far for at least one of them: a line's
// record is read at a wave-uniform address (no lists, no list positions, no clamps), every lane accumulates its own node
// (no sum across lanes), and the fraction's depth is chosen per pair of lines from the classification's own edge bound.
__device__ __forceinline__ unsigned ff_fold16(unsigned long long m) {       // OR of the four tiles' 16-bit fields
    const unsigned h = (unsigned)m | (unsigned)(m >> 32);
    return (h | (h >> 16)) & 0xffffu;
}
#if VAMP_SUPER_NODES && VAMP_DEAL_ADJ
#define VAMP_SUPER_ON 1
#include "ff_super.inc"                // FF_SUPER_C (tools/gen_ff_super.py)
#else
#define VAMP_SUPER_ON 0
#endif
// the per-batch sets of lines, nested: n6 <= n4 <= n3 <= far (bit k: line k is far for some tile of the batch and the
// deepest fraction any of those tiles needs has at least that many levels), and the lines wide for some tile.  (The lines
// distant from the batch's super-tile, VAMP_SUPER_NODES, are in none of them: ff_super_batch takes them out.)
struct NodeSets { unsigned far, n6, n4, n3, wide; };
// The classification of a FULL batch for the fp64 loop: ff_classify_batch's masks without its lists, plus the depth class
// of every far pair from r2e = (dist s)^2 + y^2.  Every node of the tile lies inside it, at least `dist` from the line's
// centre, so r2e is a lower bound of r2 at every node, and a deeper fraction is valid wherever a shallower one is.
// Leaves (mid, half) of the lane's tile j = lane >> 4 with the caller: the node pass wants them on the same lanes.
template <bool WIDE, bool ZONE, class LDS>
__device__ __forceinline__ void ff_classify_batch_np(const LDS& L, const double2* __restrict__ geo, int K, int lane_, int base, int stride,
                                                     unsigned wide_all, unsigned long long& farmasks, unsigned long long& widemasks,
                                                     unsigned long long& zonemasks, NodeSets& sets, double& mid, double& half) {
    int lane = lane_;
    asm volatile("" : "+v"(lane));
    const int j = lane >> 4, k = lane & (KMAX - 1);
    const double2 g = geo[(base + j * stride) >> 8];
    mid = g.x, half = fabs(g.y);
    const LineRec& me = *reinterpret_cast<const LineRec*>(reinterpret_cast<const char*>(L.line) +
                                                          __umul24((unsigned)(k < K ? k : 0), (unsigned)sizeof(LineRec)));
    const double my_c = me.c, my_s = me.s, my_y = me.y, my_w8 = me.w8, my_wmid = me.wmid;
    const double dist = fabs(mid - my_c) - half;
    const bool my_beyond = (k < K) & (dist >= FF_DIST * half);
    const bool my_far = my_beyond & (dist >= my_w8);
    const double Xe = dist * my_s, r2e = fma(Xe, Xe, my_y * my_y);
    farmasks = __ballot(my_far);
    sets.far = ff_fold16(farmasks);
    sets.n6 = ff_fold16(__ballot(my_far & (r2e < VAMP_FF_R2_M4)));
    sets.n4 = ff_fold16(__ballot(my_far & (r2e < VAMP_FF_R2_M3)));
    sets.n3 = ff_fold16(__ballot(my_far & (r2e < VAMP_FF_R2_M2)));
    widemasks = 0ull;
    if constexpr (WIDE) {       // (never far AND wide for one tile: the mark of a tile done from its moments, as in ff_classify_batch)
        const bool my_wide = ((((wide_all >> k) & 1u) != 0u) | (VAMP_MID_NODES && (my_beyond & (dist >= my_wmid)))) & !my_far;
        widemasks = __ballot(my_wide);
    }
    sets.wide = ff_fold16(widemasks);
    zonemasks = 0ull;
    if constexpr (ZONE) zonemasks = __ballot(vamp::ff_tile_in_zone(my_c, my_s, my_y, mid, half));
}
// The node pass: lane 16 j + n ends with the node sum of (tile j, node n) -- far lines through the fractions, two lines per
// iteration sharing a reciprocal (ff_frac2), deepest class first, M the class of the deeper of the two; then (WIDE) the
// lines wide or "mid" for some tile through their Taylor tables, ff_wide_nodes' arithmetic.  A lane for whose tile a line
// is NOT far takes X = FF_X_IDLE in its place: the parent never evaluated a fraction inside |z| < 8, and the partner's
// value shares the reciprocal.  A walker with a guard bit (GUARD) evaluates its pairs through ff_eval2<true>, which
// clamps, patches and picks the depth from the arguments themselves (the idle argument asks for the shallowest).
constexpr double FF_X_IDLE = 64.0;          // |z|^2 >= 4096: every fraction's range, and below X_FAR
static_assert(FF_X_IDLE * FF_X_IDLE >= VAMP_FF_R2_M2 && FF_X_IDLE < vamp::X_FAR, "the idle argument neither deepens a pair nor needs a guard");
template <int M> struct NpDepth { static constexpr int value = M; };       // the depth of a run of pairs (VAMP_NP_CLASS_RUNS)
#if VAMP_SUPER_ON
// The distant pass (VAMP_SUPER_NODES): the batch's distant lines (dist, and d3 <= dist, those whose edge bound on the
// super-tile (Mid, Half) asks for three levels: ff_super_batch) summed at the 16
// Chebyshev nodes of the batch's SUPER-tile and interpolated to the 64 (tile, node) points, which lane 16 j + n returns
// for its own.  Lane 16 g + n evaluates at super-node n the lines of group g: slot 4 t + g of the eight lines of an
// iteration (vamp::super_order), t = 0, 1 sharing a reciprocal as in ff_frac2; three levels while an iteration holds a
// line that asks for them, then two; a slot past the last line takes the idle argument and a zero amplitude.  The four
// groups are added in one order on every lane, the 16 sums become Chebyshev coefficients through the constant cosine
// table FF_SUPER_C (lane k forms c_k; through Sx.coef, which is free until the batch's tile loops), and every lane
// evaluates Clenshaw's recurrence at t = (xnode - Mid) / Half, the coefficients read at wave-uniform LDS addresses.
template <class LDS>
__device__ __forceinline__ double ff_super_pass(const LDS& L, TileScratch& Sx, const double* __restrict__ dct, int lane, double xnode,
                                                unsigned dist, unsigned d3, double Mid, double Half) {
    const vamp::SuperOrder ord = vamp::super_order(dist, d3);
    const int n = lane & (FF_NODES - 1), g4 = (lane >> 4) * 4;
    const double xs = fma(Half, dct[FF_MAT + n], Mid);
    unsigned long long seq = ord.seq;
    int left = ord.n;               // lines of the sequence not yet taken
    double acc = 0.0;
    auto run = [&](auto depth, int iters) {
        constexpr int M = decltype(depth)::value;
#pragma unroll 1
        for (int i = 0; i < iters; ++i) {
            const unsigned s32 = (unsigned)seq >> g4;
            double X[2], y[2], amp[2], r2[2], nn[2], d[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const LineRec& ln = *reinterpret_cast<const LineRec*>(reinterpret_cast<const char*>(L.line) +
                                                                      __umul24((s32 >> (16 * t)) & 15u, (unsigned)sizeof(LineRec)));
                const bool live = (g4 >> 2) + 4 * t < left;
                const double Xl = fabs(xs - ln.c) * ln.s;
                X[t] = live ? Xl : FF_X_IDLE;
                y[t] = ln.y;
                amp[t] = live ? ln.amp : 0.0;
                r2[t] = fma(X[t], X[t], y[t] * y[t]);
                vamp::voigt_jfrac_nd<M>(X[t], y[t], r2[t], nn[t], d[t], vamp::GHFrac<M>::Z, vamp::GHFrac<M>::C);
            }
            const double ra = vamp::rcp_nr(d[0] * d[1]);        // (ff_frac2)
            acc = fma(amp[0], nn[0] * (ra * d[1]), acc);
            acc = fma(amp[1], nn[1] * (ra * d[0]), acc);
            seq >>= 32;
            left -= 8;
        }
    };
    run(NpDepth<3>{}, ord.iters3);
    run(NpDepth<2>{}, ord.iters - ord.iters3);
    // (g0 + g1) + (g2 + g3) on every lane.  The partners' addresses are formed here, from lane_here(): taken from the
    // kernel's other cross-lane sums they were spilled in the prologue and reloaded from scratch in every batch
    {
        const int me = lane_here();
        const int a16 = (me ^ 16) << 2, a32 = (me ^ 32) << 2;
        acc += __hiloint2double(__builtin_amdgcn_ds_bpermute(a16, __double2hiint(acc)), __builtin_amdgcn_ds_bpermute(a16, __double2loint(acc)));
        acc += __hiloint2double(__builtin_amdgcn_ds_bpermute(a32, __double2hiint(acc)), __builtin_amdgcn_ds_bpermute(a32, __double2loint(acc)));
    }
    if (lane < FF_NODES) Sx.coef[lane] = acc;
    __builtin_amdgcn_wave_barrier();
    const double2* crow = reinterpret_cast<const double2*>(FF_SUPER_C) + n;
    const double2* fv = reinterpret_cast<const double2*>(Sx.coef);
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int n2 = 0; n2 < FF_NODES / 2; ++n2) {
        const double2 m = crow[n2 * FF_NODES], f2 = fv[n2];
        a0 = fma(m.x, f2.x, a0);
        a1 = fma(m.y, f2.y, a1);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < FF_NODES) Sx.coef[lane] = a0 + a1;
    __builtin_amdgcn_wave_barrier();
    const double t = (xnode - Mid) * vamp::rcp_nr(Half), t2 = t + t;
    double b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = FF_NODES - 1; k >= 1; --k) {
        const double b = fma(t2, b1, Sx.coef[k] - b2);
        b2 = b1;
        b1 = b;
    }
    const double p = fma(t, b1, Sx.coef[0] - b2);
    __builtin_amdgcn_wave_barrier();        // (the tile loops write Sx.coef next)
    return p;
}
// The distant lines of a full batch of four ADJACENT tiles, for a walker that may take the pass (no guard bit, no line wide
// for every tile: the caller's one scalar branch per batch; everything of the pass is formed behind it).  The four tiles
// as one super-tile: line k has the same verdict on all four rows of lanes, one ballot, and one for the depth; "far for
// every tile of the batch" is asked of the masks themselves, not of the rounding.  A distant line stays in farmasks -- it
// is far, not near, for the tile loops -- and leaves the sets of the ordinary pairs, from which alone ff_node_pass takes
// its lines.  Returns the distant lines' sum at (tile lane >> 4, node lane & 15), the node pass's first addend.  The
// lane's line and its tile's node are read again here and not carried over from the classification.
template <class LDS>
__device__ __forceinline__ double ff_super_batch(const LDS& L, TileScratch& Sx, const double* __restrict__ dct, const double2* __restrict__ geo,
                                                 int K, int lane_, int base, int stride, double mid, double half,
                                                 unsigned long long farmasks, NodeSets& sets) {
    int lane = lane_;
    asm volatile("" : "+v"(lane));
    const int k = lane & (KMAX - 1);
    const LineRec& me = *reinterpret_cast<const LineRec*>(reinterpret_cast<const char*>(L.line) +
                                                          __umul24((unsigned)(k < K ? k : 0), (unsigned)sizeof(LineRec)));
    const double my_c = me.c, my_s = me.s, my_y = me.y;
    const double2 g0 = geo[base >> 8], g3 = geo[(base + (FF_BATCH - 1) * stride) >> 8];
    double Mid, Half;
    vamp::ff_super_tile(g0.x, fabs(g0.y), g3.x, fabs(g3.y), Mid, Half);
    const bool my_dist = (k < K) & vamp::ff_super_distant(my_c, my_s, my_y, Mid, Half);
    const bool my_d3 = my_dist & (vamp::ff_super_r2e(my_c, my_s, my_y, Mid, Half) < VAMP_FF_R2_M2);
    const unsigned all4 = (unsigned)farmasks & (unsigned)(farmasks >> 16) & (unsigned)(farmasks >> 32) & (unsigned)(farmasks >> 48) & 0xffffu;
    const unsigned dist = (unsigned)__ballot(my_dist) & all4;
    if (dist == 0u) return 0.0;
    const unsigned d3 = (unsigned)__ballot(my_d3) & dist;
    sets.far &= ~dist, sets.n6 &= ~dist, sets.n4 &= ~dist, sets.n3 &= ~dist;
    const double xnode = fma(half, dct[FF_MAT + (lane & (FF_NODES - 1))], mid);
    return ff_super_pass(L, Sx, dct, lane, xnode, dist, d3, Mid, Half);
}
#endif
// (fs0: what the lane's sum starts from -- ff_super_batch's share of it, or zero)
template <bool WIDE, bool GUARD, class LDS>
__device__ __forceinline__ double ff_node_pass(const LDS& L, const double* __restrict__ dct, const double* tab, int lane_, double mid, double half,
                                               unsigned long long farmasks, unsigned long long widemasks, NodeSets sets, double fs0 = 0.0) {
    int lane = lane_;
    asm volatile("" : "+v"(lane));
    const double xnode = fma(half, dct[FF_MAT + (lane & (FF_NODES - 1))], mid);
    double fs = fs0;
    const unsigned far16 = ff_tile_field(farmasks, lane);
#if VAMP_NP_CLASS_RUNS
    // The pairs in vamp::np_pair_order's order, as one counted loop per depth: the constants of a depth are read once ahead
    // of its loop and serve both values of every pair of the run.  The records of a pair are read at their wave-uniform
    // addresses by every lane, one pair ahead of their use, and a lane for whose tile a line is not far selects the idle
    // argument and a zero amplitude: the values of the branches these replace.  (Past the last pair the sequence holds
    // zeros: the read ahead takes line 0 and nobody uses it.)
    if (sets.far != 0u) {       // (a batch without a far line -- every line wide, the prior's walkers -- pays one branch, as before)
    const vamp::NpOrder ord = vamp::np_pair_order(sets.far, sets.n6, sets.n4, sets.n3);
    unsigned long long seq = ord.seq;
    const unsigned far16b = far16 & ~ord.solo;          // the second slot of a line paired with itself adds nothing
    struct Pair { double c[2], s[2], y[2], amp[2]; };
    auto read_pair = [&](unsigned long long q) {
        Pair p;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const LineRec& ln = L.line[(unsigned)(q >> (4 * t)) & 15u];
            p.c[t] = ln.c, p.s[t] = ln.s, p.y[t] = ln.y, p.amp[t] = ln.amp;
        }
        return p;
    };
    Pair nxt = read_pair(seq);
    auto run = [&](auto depth, int npairs, const double* Zt, const double* Ct) {
        constexpr int M = decltype(depth)::value;
#pragma unroll 1
        for (int i = 0; i < npairs; ++i) {
            const Pair p = nxt;
            const unsigned k0 = (unsigned)seq & 15u, k1 = (unsigned)(seq >> 4) & 15u;
            seq >>= 8;
            nxt = read_pair(seq);
            const bool mine[2] = {((far16 >> k0) & 1u) != 0u, ((far16b >> k1) & 1u) != 0u};
            double X[2], amp[2], H[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const double Xl = fabs(xnode - p.c[t]) * p.s[t];
                X[t] = mine[t] ? Xl : FF_X_IDLE;
                amp[t] = mine[t] ? p.amp[t] : 0.0;
            }
            if constexpr (GUARD) {
                ff_eval2<true>(X, p.y, H, dct + FF_EXP);
            } else {
                const double r2[2] = {fma(X[0], X[0], p.y[0] * p.y[0]), fma(X[1], X[1], p.y[1] * p.y[1])};
                double n[2], d[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) vamp::voigt_jfrac_nd<M>(X[t], p.y[t], r2[t], n[t], d[t], Zt, Ct);
                const double ra = vamp::rcp_nr(d[0] * d[1]);        // (ff_frac2)
                H[0] = n[0] * (ra * d[1]);
                H[1] = n[1] * (ra * d[0]);
            }
            fs = fma(amp[0], H[0], fs);
            fs = fma(amp[1], H[1], fs);
        }
    };
    if constexpr (GUARD) {          // (ff_eval2 picks the depth from the arguments: one run)
        run(NpDepth<2>{}, ord.pairs[0] + ord.pairs[1] + ord.pairs[2] + ord.pairs[3], nullptr, nullptr);
    } else {
        // (the opaque zero stands between a run's constants and the runs before it: read ahead of ITS loop, no earlier)
        const int z6 = vamp::opaque_zero();
        run(NpDepth<6>{}, ord.pairs[0], vamp::GHFrac<6>::Z + z6, vamp::GHFrac<6>::C + z6);
        const int z4 = vamp::opaque_zero();
        run(NpDepth<4>{}, ord.pairs[1], vamp::GHFrac<4>::Z + z4, vamp::GHFrac<4>::C + z4);
        run(NpDepth<3>{}, ord.pairs[2], vamp::GHFrac<3>::Z, vamp::GHFrac<3>::C);
        run(NpDepth<2>{}, ord.pairs[3], vamp::GHFrac<2>::Z, vamp::GHFrac<2>::C);
    }
    }
#else
    unsigned rest = sets.far, n6 = sets.n6, n4 = sets.n4, n3 = sets.n3;
    while (rest) {
        const int depth = n6 ? 6 : n4 ? 4 : n3 ? 3 : 2;
        int kk[2];
        bool live[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {               // the next line of the deepest class that has one; an odd last line pairs
            live[t] = rest != 0u;                   // with a copy of itself that no lane adds
            if (live[t]) {
                kk[t] = __builtin_ctz(n6 ? n6 : n4 ? n4 : n3 ? n3 : rest);
                const unsigned keep = ~(1u << kk[t]);
                rest &= keep, n6 &= keep, n4 &= keep, n3 &= keep;
            } else {
                kk[t] = kk[0];
            }
        }
        double X[2], y[2], amp[2], H[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const LineRec& ln = L.line[kk[t]];
            const bool mine = live[t] & (((far16 >> kk[t]) & 1u) != 0u);
            X[t] = mine ? fabs(xnode - ln.c) * ln.s : FF_X_IDLE;
            y[t] = ln.y;
            amp[t] = mine ? ln.amp : 0.0;
        }
        if constexpr (GUARD) {
            ff_eval2<true>(X, y, H, dct + FF_EXP);
        } else {
            const double r2[2] = {fma(X[0], X[0], y[0] * y[0]), fma(X[1], X[1], y[1] * y[1])};
            if (depth == 6) ff_frac2<6>(X, y, r2, H);
            else if (depth == 4) ff_frac2<4>(X, y, r2, H);
            else if (depth == 3) ff_frac2<3>(X, y, r2, H);
            else ff_frac2<2>(X, y, r2, H);
        }
        fs = fma(amp[0], H[0], fs);
        fs = fma(amp[1], H[1], fs);
    }
#endif
    if constexpr (WIDE) {
        const unsigned wide16 = ff_tile_field(widemasks, lane);
        for (unsigned w = sets.wide; w; w &= w - 1u) {
            const int k = __builtin_ctz(w);
            if ((wide16 >> k) & 1u) {
                const LineRec& ln = L.line[k];
                const double X = fabs(xnode - ln.c) * ln.s, r2 = fma(X, X, ln.y * ln.y);
                double H;
                if (r2 < vamp::R2_CORE) {
                    H = table_eval(tab + k * vamp::TAB_LINE, X);
                } else {
                    H = vamp::voigt_jfrac<6>(X, ln.y, r2);
                    if (ln.y < vamp::Y_TINY) H += vamp::SQRT_PI * vamp::exp_neg_sq_tab(X, dct + FF_EXP);
                }
                fs = fma(ln.amp, H, fs);
            }
        }
    }
    return fs;
}
// ff_series for a value every lane holds for (tile lane >> 4, node lane & 15): row `j` hands over its tile's node values
template <class real>
__device__ __forceinline__ void ff_series_row(TileScratch& Sx, const double* __restrict__ dct, int lane, int j, double fs) {
#if VAMP_SUPER_ON
    // (the lane's node index is formed here: shared with the kernel's prologue it was spilled there, once the distant
    //  pass stood in the batch loop, and reloaded from scratch in every tile)
    asm volatile("" : "+v"(lane));
#endif
    if ((lane >> 4) == j) Sx.coef[lane & (FF_NODES - 1)] = fs;
    __builtin_amdgcn_wave_barrier();
    const double2* mrow = reinterpret_cast<const double2*>(dct) + (lane < FF_ROWS ? lane : FF_ROWS - 1);
    const double2* fv = reinterpret_cast<const double2*>(Sx.coef);
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int n2 = 0; n2 < FF_NODES / 2; ++n2) {
        const double2 m = mrow[n2 * FF_ROWS], f2 = fv[n2];
        a0 = fma(m.x, f2.x, a0);
        a1 = fma(m.y, f2.y, a1);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < FF_ROWS) reinterpret_cast<real*>(Sx.coef)[lane] = (real)(a0 + a1);
    __builtin_amdgcn_wave_barrier();
}
// ff_moment_chi_nodes for the absorption every lane holds for (tile lane >> 4, node lane & 15): row `j` hands its 16
// values over through Sx.coef, and every lane takes its own a_n from there with the a_m of its columns
__device__ __forceinline__ void ff_moment_chi_nodes_row(TileScratch& Sx, const double* __restrict__ mt, int lane, int j, double a_row, double c0,
                                                        double& chi) {
    if ((lane >> 4) == j) Sx.coef[lane & (FF_NODES - 1)] = a_row;
    const int n = lane & (FF_NODES - 1), g4 = (lane >> 4) * 4;
    const double2* Qr = reinterpret_cast<const double2*>(mt + vamp::FFN_Q + n * FF_NODES + g4);
    const double2 q01 = Qr[0], q23 = Qr[1];
    const double Sv = mt[vamp::FFN_S + n];
    __builtin_amdgcn_wave_barrier();
    const double2* av = reinterpret_cast<const double2*>(Sx.coef + g4);
    const double2 a01 = av[0], a23 = av[1];
    const double a = Sx.coef[n];
    const double acc0 = fma(q01.x, a01.x, 0.5 * Sv), acc1 = q01.y * a01.y;
    const double term = a * (fma(q23.x, a23.x, acc0) + fma(q23.y, a23.y, acc1));
    chi += lane == 0 ? term + c0 : term;
    __builtin_amdgcn_wave_barrier();
}
// sweep_range_ff with the node stage of every FULL batch done line by line ahead of the batch's tile loops; what is left
// of the range after its full batches -- all of a range of fewer than FF_BATCH tiles -- goes through sweep_range_ff
// itself.  Without VAMP_DEAL_ADJ tile order and the per-lane order of the chi additions are sweep_range_ff's; with it a
// class's batches are four adjacent tiles each (see the loop's head), on every shape alike.  The near lines, the series,
// Horner's rule and the exponentials are its arithmetic; the node values differ by the order of their sums and, where a
// pair is evaluated deeper than before, by the fractions' own differences (1e-13 of a value).
template <int MODE, class PK, bool TAB, bool WIDE = false, bool GUARD = true, bool SUPER = false>
__device__ __forceinline__ void sweep_range_ff_np(const RegionDev& R, const typename PK::Lds& L, TileScratch& Sx, const double* __restrict__ dct,
                                                  const double* __restrict__ x, const double* __restrict__ f,
                                                  const double* __restrict__ wt, const double* __restrict__ ut,
                                                  const double2* __restrict__ geo, int lane, int base0, int base1, int stride,
                                                  double& chi, const double* tab, unsigned long long wide_all = 0ull,
                                                  const double* __restrict__ mom = nullptr) {
    constexpr int T = TPIX;
    static_assert(PK::LPW == 64 && PK::KCAP <= 16, "far-field tiles: one walker per wavefront, <= 16 lines");
    const int K = R.K;
    const int ntile = base0 < base1 ? (base1 - base0 + stride - 1) / stride : 0;
    // (a wavefront's range is wave-uniform, and so are the batch loop's bounds: said here, because where the range comes
    //  from the wavefront's index the compiler takes the loop for a divergent one and keeps its counter in a vector register)
#if VAMP_DEAL_ADJ
    // (base0, stride) name class p = base0 / tile of the stride / tile classes of a region whose first tile is pixel 0.  A
    // whole group of stride / tile batches of FF_BATCH ADJACENT tiles gives the class its p-th batch; the tiles no group
    // holds, fewer than a group, are the class's p, p + stride, .. of them and go tile by tile through sweep_range_ff.
    (void)ntile;
    const int tstride = 64 * T, bstep = FF_BATCH * stride;
    const int bfull = __builtin_amdgcn_readfirstlane((base1 / bstep) * bstep);                                  // the first tile past the whole groups
    const int bfirst = FF_BATCH * base0, brest = bfull + base0;
#else
    const int tstride = stride, bstep = FF_BATCH * stride;
    const int bfull = __builtin_amdgcn_readfirstlane(base0 + (ntile / FF_BATCH) * (FF_BATCH * stride));       // the first tile past the full batches
    const int bfirst = base0, brest = bfull;
#endif
    for (int batch = __builtin_amdgcn_readfirstlane(bfirst); batch < bfull; batch += bstep) {
    unsigned long long farmasks, widemasks, zonemasks;
    double fsn;         // node sum of (tile lane >> 4, node lane & 15): one register pair across the batch's tile loops
    {
        NodeSets sets;
        double mid_j, half_j;
        ff_classify_batch_np<WIDE, TAB>(L, geo, K, lane, batch, tstride, (unsigned)wide_all, farmasks, widemasks, zonemasks, sets, mid_j, half_j);
#if VAMP_SUPER_ON
        // (SUPER: no guard bit.  Whether the walker takes the distant pass is a function of the walker alone -- no line wide for
        //  every tile -- and wave-uniform, said as the loop's bounds are.  It is asked of the flags here, in every batch:
        //  formed once ahead of the loop it is one scalar more across the loop, and the prior ensemble, whose walkers never
        //  take the pass, ran 1.4 % slower; profiles/super_nodes_on_ab.txt)
        double fs0 = 0.0;
        if constexpr (SUPER) {
            if (__builtin_amdgcn_readfirstlane((int)(unsigned)wide_all) == 0) {
                fs0 = ff_super_batch(L, Sx, dct, geo, K, lane, batch, tstride, mid_j, half_j, farmasks, sets);
            }
        }
        fsn = ff_node_pass<WIDE, GUARD>(L, dct, tab, lane, mid_j, half_j, farmasks, widemasks, sets, fs0);
#else
        fsn = ff_node_pass<WIDE, GUARD>(L, dct, tab, lane, mid_j, half_j, farmasks, widemasks, sets);
#endif
    }
#if VAMP_TILE_MOMENTS == 2
    {   // tiles without a near line (see sweep_range_ff).  The absorption at the nodes and its largest value per tile are
        // formed once for the batch, when the first tile asks.  ff_moments_try still turns a tile away on the data alone:
        // the node stage it used to spare is done by now, but on data the form never suits (weights of 1e10) it spares
        // the batch the exponential, the row maxima and a record's loads
        unsigned long long fm = farmasks, wm = widemasks;
        double a_row = 0.0, amax_row = 0.0;
        bool have_a = false;
#pragma unroll 1
        for (int j = 0; j < FF_BATCH; ++j, fm >>= KMAX, wm >>= KMAX) {
            const unsigned farmask = (unsigned)fm & 0xffffu, widemask = WIDE ? (unsigned)wm & 0xffffu : 0u;
            if ((~(farmask | widemask) & ((1u << K) - 1u)) != 0u) continue;
            const double* mt = mom + ((batch + j * tstride) >> 8) * MOM_TILE;
            const double root_c0 = mt[MOM_RC], root_q0 = mt[MOM_RQ];
            if (!vamp::ff_moments_try(root_c0, root_q0)) continue;
            if (!have_a) {
                int eoff = FF_EXP;
                asm volatile("" : "+s"(eoff));
                a_row = -vamp::expm1_taylor_tab(-fsn, dct + eoff);
                amax_row = row16_max(fabs(a_row));
                have_a = true;
            }
            const double amax = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(amax_row), KMAX * j),
                                                 __builtin_amdgcn_readlane(__double2loint(amax_row), KMAX * j));
            if (!vamp::ff_moments_ok(root_c0, root_q0, amax)) continue;
            ff_moment_chi_nodes_row(Sx, mt, lane_here(), j, a_row, mt[vamp::FFN_C0], chi);
            const unsigned long long field = 0xffffull << (KMAX * j);
            farmasks |= field;
            widemasks |= field;
        }
    }
#endif
#pragma unroll 1
    for (int j = 0; j < FF_BATCH; ++j, farmasks >>= KMAX, widemasks >>= KMAX, zonemasks >>= KMAX) {
        const int base = batch + j * tstride;
        double xi[T], tau[T];
#if VAMP_TILE_HEAD
        if ((unsigned)farmasks & (unsigned)widemasks & 0xffffu) continue;      // done from its moments: nothing of it is loaded
#endif
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xi[t] = x[base + 64 * t + lane];
            tau[t] = 0.0;
        }
#if !VAMP_TILE_HEAD
        if ((unsigned)farmasks & (unsigned)widemasks & 0xffffu) continue;      // done from its moments
#endif
        const bool up = __double2hiint(geo[base >> 8].y) >= 0;
        const unsigned farmask = (unsigned)farmasks & 0xffffu;
        const unsigned widemask = WIDE ? (unsigned)widemasks & 0xffffu : 0u;
        for (unsigned near = ~(farmask | widemask) & ((1u << K) - 1u); near; near &= near - 1u) {
            const int k = __builtin_ctz(near);
            const LineRec ln = L.line[k];
            double X[T], H[T];
#pragma unroll
            for (int t = 0; t < T; ++t) X[t] = fabs(xi[t] - ln.c) * ln.s;
            if (TAB && (((unsigned)zonemasks >> k) & 1u)) {
                table_eval_tile<T>(tab + k * vamp::TAB_LINE, X, H);
            } else {
                tile_voigt<T, TAB>(ln, dtab_row<PK>(L, k), X, H, TAB ? tab + k * vamp::TAB_LINE : nullptr, dct + FF_EXP);
            }
#pragma unroll
            for (int t = 0; t < T; ++t) tau[t] = fma(ln.amp, H[t], tau[t]);
        }
        double fi[T], wi[T];
        if ((farmask | widemask) != 0u) {
            // the pixels' places in their quarters: xi has ended with the near lines, u takes its registers; the
            // transform's LDS reads stand between the request and Horner's rule
            double u[T];
#pragma unroll
            for (int t = 0; t < T; ++t) u[t] = ut[base + 64 * t + lane];
            ff_series_row<double>(Sx, dct, lane, j, fsn);
#if VAMP_EARLY_LOADS
#pragma unroll
            for (int t = 0; t < T; ++t) {
                fi[t] = f[base + 64 * t + lane];
                wi[t] = wt[base + 64 * t + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
#endif
            ff_horner<double, T>(Sx, u, up, tau);
        } else {
#if VAMP_EARLY_LOADS
#pragma unroll
            for (int t = 0; t < T; ++t) {
                fi[t] = f[base + 64 * t + lane];
                wi[t] = wt[base + 64 * t + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
#endif
        }
        int eoff = FF_EXP;
        asm volatile("" : "+s"(eoff));          // (as in sweep_range_ff: the exp constants are read per tile, not kept)
        const double* ec = dct + eoff;
#pragma unroll
        for (int t = 0; t < T; ++t) {
#if !VAMP_EARLY_LOADS
            fi[t] = f[base + 64 * t + lane];
            wi[t] = wt[base + 64 * t + lane];
#endif
            const double m = vamp::exp_taylor_tab<VAMP_FLUX_EXP_DROP>(-tau[t], ec);
            const double r = (fi[t] - m) * wi[t];
            chi = fma(r, r, chi);
        }
    }
    }
    if (brest < base1) sweep_range_ff<MODE, PK, TAB, WIDE, GUARD>(R, L, Sx, dct, x, f, wt, ut, geo, lane, brest, base1, stride, chi, tab, wide_all, mom);
}
#endif
#ifndef VAMP_SUPER_ON
#define VAMP_SUPER_ON 0
#endif
// the fp64 far-field sweep of a range as the library was built
// (SUPER: the loop of the walkers without a guard bit, which holds the distant pass; a walker with a line wide for every
//  tile runs the same loop and skips the pass at one scalar branch per batch)
template <int MODE, class PK, bool TAB, bool WIDE, bool GUARD, bool SUPER = false, class... Args>
__device__ __forceinline__ void sweep_range_ff_any(Args&&... args) {
#if VAMP_NODE_PASS_ON
    static_assert(!(SUPER && GUARD), "a guard walker keeps the ordinary pass");
    sweep_range_ff_np<MODE, PK, TAB, WIDE, GUARD, SUPER && VAMP_SUPER_ON>(static_cast<Args&&>(args)...);
#else
    sweep_range_ff<MODE, PK, TAB, WIDE, GUARD>(static_cast<Args&&>(args)...);
#endif
}

#ifndef VAMP_FARFIELD
#define VAMP_FARFIELD 1
#endif

// fp32 pixel arithmetic (Humlicek W4), chi^2 accumulated in fp64 (SURVEY section 7 hard parts).
// Same shape as the fp64 sweep: TPIX pixels per lane in full tiles and one region per (tile, line) and walker
// group (group_any) -- region I when every lane has s >= 15, region II (valid for all s >= 5.5) when every lane
// has s >= 5.5, per-lane selection only for tiles that touch the line core.
template <int T, int LPW = 64>
__device__ __forceinline__ void tile_w4(float y, const float (&X)[T], float (&H)[T]) {
    float lo = X[0];
#pragma unroll
    for (int t = 1; t < T; ++t) lo = fminf(lo, X[t]);
    lo += y;
    if (!group_any<LPW>(!(lo >= 15.0f))) {
#pragma unroll
        for (int t = 0; t < T; ++t) H[t] = vamp::w4_region1(X[t], y);
    } else if (!group_any<LPW>(!(lo >= 5.5f))) {
#pragma unroll
        for (int t = 0; t < T; ++t) H[t] = vamp::w4_region2(X[t], y);
    } else {
#pragma unroll
        for (int t = 0; t < T; ++t) H[t] = vamp::humlicek_w4_re(X[t], y);
    }
}

// the same with the line's fp32 Taylor rows for |z|^2 < 64 (the zone the far-field classification calls a line's
// core): region I / II outside it (|z| >= 8 implies s >= 5.5), one table look-up per pixel inside
__device__ __forceinline__ float table32_eval(const float* tab, float x) {
    // interval i = floor(2 x) as round-to-nearest of 2 (x - 1/4): adding 2^23 + 2^22 leaves the integer in the low
    // bits of the sum (no conversions); on a boundary either neighbour is right (|d| = 1/4 in both)
    constexpr float MAGIC = 12582912.0f;
    const float xs = x - 0.25f;
    const float t = fmaf(xs, 2.0f, MAGIC);
    const int i = __float_as_int(t) & 15;
    const float d = fmaf(t - MAGIC, -0.5f, xs);
    const float4* a = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tab) + i * (vamp::TAB32_NT * (int)sizeof(float)));
    const float4 lo = a[0], hi = a[1];
    float r = fmaf(hi.w, d, hi.z);
    r = fmaf(r, d, hi.y);
    r = fmaf(r, d, hi.x);
    r = fmaf(r, d, lo.w);
    r = fmaf(r, d, lo.z);
    r = fmaf(r, d, lo.y);
    return fmaf(r, d, lo.x);
}
template <int T>
__device__ __forceinline__ void tile_w4_tab(float y, const float (&X)[T], float (&H)[T], const float* tab) {
    float lo = X[0];
#pragma unroll
    for (int t = 1; t < T; ++t) lo = fminf(lo, X[t]);
    const float y2 = y * y;
    if (!__any(!(lo + y >= 15.0f))) {
#pragma unroll
        for (int t = 0; t < T; ++t) H[t] = vamp::w4_region1(X[t], y);
    } else if (!__any(!(fmaf(lo, lo, y2) >= (float)vamp::R2_CORE))) {
#pragma unroll
        for (int t = 0; t < T; ++t) H[t] = vamp::w4_region2(X[t], y);
    } else {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (fmaf(X[t], X[t], y2) < (float)vamp::R2_CORE) H[t] = table32_eval(tab, X[t]);
            else H[t] = vamp::w4_region2(X[t], y);
        }
    }
}

template <int MODE, class PK, int T>
__device__ __forceinline__ void sweep_range_f32(const RegionDev& R, const typename PK::Lds& L, const float* __restrict__ x,
                                                const float* __restrict__ f, const float* __restrict__ wt, int lane,
                                                int base0, int base1, int stride, double& chi) {
    const int K = R.K, P = R.P;
    constexpr bool gauss = (MODE == VAMP_GAUSS3);
    constexpr int LPW = PK::LPW;
    for (int base = base0; base < base1; base += stride) {
        float xi[T], tau[T];
        int idx[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int i = base + LPW * t + lane;
            idx[t] = i < P ? i : P - 1;
            xi[t] = x[idx[t]];
            tau[t] = 0.0f;
        }
        for (int k = 0; k < K; ++k) {
            const float c = L.linef[k][0], s = L.linef[k][1], y = L.linef[k][2], a = L.linef[k][3];
            if constexpr (gauss) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float u = (xi[t] - c) * s;
                    tau[t] += a * __expf(-0.5f * (u * u));
                }
            } else {
                float X[T], H[T];
#pragma unroll
                for (int t = 0; t < T; ++t) X[t] = fabsf(xi[t] - c) * s;
                tile_w4<T, PK::LPW>(y, X, H);
#pragma unroll
                for (int t = 0; t < T; ++t) tau[t] = fmaf(a, H[t], tau[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const float m = __expf(-tau[t]);
            const float r = (f[idx[t]] - m) * wt[idx[t]];
            const bool live = (base + LPW * t + lane) < P;
            chi += live ? (double)r * (double)r : 0.0;
        }
    }
}

// ---- far field of fp32 contexts: 8 nodes ------------------------------------------------------------
// Single precision holds 6e-8; an 8-node (degree-7) Chebyshev interpolant already reproduces the optical depth of
// a line >= FF_DIST half-widths beyond the tile's edge to 3e-7 (tests/test_ff_matrix.py), so the fp32 path uses
// that instead of the 16-node one: lane = 8 (line slot) + node, two lines per lane, node sums over three xor
// shuffles, a 32 x 8 float matrix (row sums <= 3.4: no conditioning problem in fp32) -> four local series of 8
// coefficients, 7 multiply-adds per pixel.  Node values through W4 regions I / II (every far point has |z| >= 8).
template <class LDS>
__device__ __forceinline__ void ff32_coefficients(const LDS& L, TileScratch& Sx, const unsigned char* farlist, const float* __restrict__ dct32,
                                                  int lane, int nfar, double mid, double half) {
    const int node = lane & (FF32_NODES - 1), grp = lane >> 3;
    const float tnode = dct32[FF32_MAT + node];                    // cos(pi (node + 1/2) / 8)
    __builtin_amdgcn_wave_barrier();
    const float xn = (float)fma(half, (double)tnode, mid);
    float X[2], yv[2], av[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int q = 8 * t + grp;
        const float* lf = L.linef[farlist[q < nfar ? q : nfar - 1]];
        X[t] = fabsf(xn - lf[0]) * lf[1];
        yv[t] = lf[2];
        av[t] = q < nfar ? lf[3] : 0.0f;
    }
    float fs;
    if (nfar > 8) {
        const float lo = fminf(X[0] + yv[0], X[1] + yv[1]);
        if (!__any(!(lo >= 15.0f))) fs = fmaf(av[0], vamp::w4_region1(X[0], yv[0]), av[1] * vamp::w4_region1(X[1], yv[1]));
        else fs = fmaf(av[0], vamp::w4_region2(X[0], yv[0]), av[1] * vamp::w4_region2(X[1], yv[1]));
    } else {
        if (!__any(!(X[0] + yv[0] >= 15.0f))) fs = av[0] * vamp::w4_region1(X[0], yv[0]);
        else fs = av[0] * vamp::w4_region2(X[0], yv[0]);
    }
    fs += __shfl_xor(fs, 8, 64);
    fs += __shfl_xor(fs, 16, 64);
    fs += __shfl_xor(fs, 32, 64);
    // node sums (lanes 0..7 hold them) -> the four local series: lane l = 8 q + j < 32 owns coefficient j of quarter q
    float* cf = reinterpret_cast<float*>(Sx.coef);
    if (lane < FF32_NODES) cf[lane] = fs;
    __builtin_amdgcn_wave_barrier();
    const float4* mrow = reinterpret_cast<const float4*>(dct32) + (lane < FF32_ROWS ? lane : FF32_ROWS - 1);
    const float4* fv = reinterpret_cast<const float4*>(Sx.coef);
    const float4 m0 = mrow[0], m1 = mrow[FF32_ROWS], f0 = fv[0], f1 = fv[1];
    float a0 = m0.x * f0.x, a1 = m0.y * f0.y;
    a0 = fmaf(m0.z, f0.z, a0); a1 = fmaf(m0.w, f0.w, a1);
    a0 = fmaf(m1.x, f1.x, a0); a1 = fmaf(m1.y, f1.y, a1);
    a0 = fmaf(m1.z, f1.z, a0); a1 = fmaf(m1.w, f1.w, a1);
    __builtin_amdgcn_wave_barrier();
    if (lane < FF32_ROWS) cf[lane] = a0 + a1;
    __builtin_amdgcn_wave_barrier();
}
// Horner's rule at the tile's pixels (register t of a lane = pixel 64 t + lane: quarter t of an ascending grid)
template <int T>
__device__ __forceinline__ void ff32_horner(const TileScratch& Sx, const float (&u)[T], bool up, float (&tau)[T]) {
    static_assert(T == 4, "one pixel per quarter of the tile");
    float acc[T];
    const float* cq[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int q = up ? t : T - 1 - t;
        cq[t] = reinterpret_cast<const float*>(Sx.coef) + q * (FF32_DEG + 1);
        acc[t] = cq[t][FF32_DEG];
    }
#pragma unroll
    for (int j = FF32_DEG - 1; j >= 0; --j) {
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = fmaf(acc[t], u[t], cq[t][j]);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) tau[t] += acc[t];
    __builtin_amdgcn_wave_barrier();
}

// fp32 sweep of full tiles with the far field: near lines through W4 in fp32, all far lines through
// the tile's interpolant -- node values and cosine transform in fp64 (one evaluation per lane,
// same code as the fp64 path), transform in fp64, Horner per pixel in fp32.
template <int MODE, class PK, bool TAB32>
__device__ __forceinline__ void sweep_range_f32_ff(const RegionDev& R, const typename PK::Lds& L, TileScratch& Sx,
                                                   const double* __restrict__ dct, const float* __restrict__ x,
                                                   const float* __restrict__ f, const float* __restrict__ wt,
                                                   const float* __restrict__ ut, const double2* __restrict__ geo, int lane,
                                                   int base0, int base1, int stride, double& chi, const float* tab32) {
    constexpr int T = TPIX;
    static_assert(PK::LPW == 64 && PK::KCAP <= 16 && MODE != VAMP_GAUSS3, "far-field tiles: one walker per wavefront, Voigt lines");
    const int K = R.K;
    for (int batch = base0; batch < base1; batch += FF_BATCH * stride) {
    // (fp32: the node values are W4 regions I / II, valid from |x| + y = 5.5 -- no |z| >= 8 condition as for the fp64
    //  fractions: a line is far once the tile is outside its Gaussian core, |z|^2 >= VAMP_MID_Z2)
    unsigned long long farmasks, widemasks;
    unsigned long long zonemasks;      // (fp64 loop only: constant zero here)
    ff_classify_batch<false, true>(L, Sx, geo, K, lane, batch, base1, stride, 0u, farmasks, widemasks, zonemasks);
#pragma unroll 1
    for (int j = 0; j < FF_BATCH; ++j, farmasks >>= KMAX) {
        const int base = batch + j * stride;
        if (base >= base1) break;
        float xi[T], tau[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xi[t] = x[base + 64 * t + lane];
            tau[t] = 0.0f;
        }
        const double2 tg = geo[base >> 8];        // (as in sweep_range_ff)
        const double mid = tg.x, half = fabs(tg.y);
        const bool up = __double2hiint(tg.y) >= 0;
        const unsigned farmask = (unsigned)farmasks & 0xffffu;
        const int nfar = __builtin_popcount(farmask);
        // (VAMP_SKIP_*: timing-only builds of tools/variants.py -- the phase split in profiles/)
#ifndef VAMP_SKIP_NEAR
        for (unsigned near = ~farmask & ((1u << K) - 1u); near; near &= near - 1u) {
            const int k = __builtin_ctz(near);
            const float c = L.linef[k][0], sc = L.linef[k][1], y = L.linef[k][2], a = L.linef[k][3];
            float X[T], H[T];
#pragma unroll
            for (int t = 0; t < T; ++t) X[t] = fabsf(xi[t] - c) * sc;
            if constexpr (TAB32) tile_w4_tab<T>(y, X, H, tab32 + k * vamp::TAB32_LINE);
            else tile_w4<T>(y, X, H);
#pragma unroll
            for (int t = 0; t < T; ++t) tau[t] = fmaf(a, H[t], tau[t]);
        }
#endif
        if (nfar > 0) {
            float u[T];             // requested ahead of the node stage that hides the round trip
#pragma unroll
            for (int t = 0; t < T; ++t) u[t] = ut[base + 64 * t + lane];
#ifndef VAMP_SKIP_FFNODES
            ff32_coefficients<typename PK::Lds>(L, Sx, Sx.farlist[j], reinterpret_cast<const float*>(dct), lane, nfar, mid, half);
#endif
#ifndef VAMP_SKIP_CLENSHAW
            ff32_horner<T>(Sx, u, up, tau);
#endif
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int i = base + 64 * t + lane;
#ifdef VAMP_SKIP_EXP
            const float m = 1.0f - tau[t];
#else
            const float m = __expf(-tau[t]);
#endif
            const float r = (f[i] - m) * wt[i];
            chi += (double)r * (double)r;
        }
    }
    }
}

struct PixPtrs {
    const double* x; const double* f; const double* wt;       // fp64 copies
    const float* xf; const float* ff; const float* wtf;       // fp32 copies (may be null)
    // far-field tables of the full tiles (k_tile_tables; null when no region has one): the pixels' places in their
    // quarters, indexed like x (fp64 contexts: u, fp32 contexts: uf), and (mid, +-half) of the tile that starts at
    // global pixel g in geo[g >> 8]
    const double* u; const float* uf; const double2* geo;
    const double* mom;      // fp64 contexts: the record of the tile in geo's slot s at mom + s MOM_TILE (ff_moments.hpp), or null
};

// The far-field tables of a context, built once per vamp_set_regions: what the tile loop used to recompute for every
// (walker, tile) though it depends on the region's abscissae alone.  Workgroup (tile, region), one thread per pixel.
//   geo[(pix_off + base) >> 8] = (mid, +-half) of the full tile at `base` -- a region's full tiles never share a slot with
//       another region's, whatever pix_off -- with the grid's orientation in the sign of half (+: ascending);
//   u[pix_off + i] (fp32 contexts: uf) = the pixel's place in its quarter of the tile, in the arithmetic ff_horner /
//       ff32_horner had for it (same device functions: a hardware reciprocal has no host twin); 0 past the last full tile.
template <bool F32>
__global__ __launch_bounds__(64 * TPIX) void k_tile_tables(const RegionDev* __restrict__ regions, const double* __restrict__ x,
                                                           const float* __restrict__ xf, double* __restrict__ u, float* __restrict__ uf,
                                                           double2* __restrict__ geo, const double* __restrict__ f = nullptr,
                                                           const double* __restrict__ wt = nullptr, double* __restrict__ mom = nullptr) {
    const RegionDev& R = regions[blockIdx.y];
    const int base = (int)blockIdx.x * (64 * TPIX), i = base + (int)threadIdx.x;
    if (i >= R.P) return;
    const long long g = R.pix_off + i;
    if (base + 64 * TPIX > R.P) {           // the tail: never read through the tables
        if constexpr (F32) uf[g] = 0.0f;
        else u[g] = 0.0;
        return;
    }
    const long long g0 = R.pix_off + base, g1 = g0 + 64 * TPIX - 1;
    const double x_lo = F32 ? (double)xf[g0] : x[g0], x_hi = F32 ? (double)xf[g1] : x[g1];
    const double mid = 0.5 * (x_lo + x_hi), half = 0.5 * fabs(x_hi - x_lo);
    const bool up = x_hi > x_lo;
    const int t = (int)threadIdx.x >> 6, q = up ? t : TPIX - 1 - t;
    double ug = 0.0;
    if constexpr (F32) {
        const float hf = (float)half, mf = (float)mid;
        const float scale = 4.0f * __builtin_amdgcn_rcpf(hf);
        uf[g] = (xf[g] - fmaf(hf, 0.5f * q - 0.75f, mf)) * scale;
    } else {
        const double scale = 4.0 * vamp::rcp_nr(half);     // (a last-bit error in the scale moves u by 1e-16)
        ug = (x[g] - fma(half, 0.5 * q - 0.75, mid)) * scale;
        u[g] = ug;
    }
    if (threadIdx.x == 0) geo[g0 >> 8] = make_double2(mid, up ? half : -half);
#if VAMP_TILE_MOMENTS == 2
    // node record of the tile (ff_moments.hpp).  The Lagrange basis of the 16 nodes t_n at the pixel's t = (x - mid) / half
    // in its barycentric form, l_n = (w_n / (t - t_n)) / sum_m w_m / (t - t_m) with w_n = (-1)^n sqrt((1 - t_n)(1 + t_n));
    // a pixel AT a node has l = 1 there and 0 elsewhere.  Then thread (n, m) sums w^2 (l_n l_m) over the tile's 256 pixels
    // (eight chains over the pixels i = k mod 8, added as a tree: one fixed order, and Q' symmetric to the bit), threads
    // 0 .. 15 sum S' as well.  C0 and sum w^2 -- what is left of chi^2 where the absorption is shallow -- in wave_sum's tree.
    if constexpr (!F32) {
        constexpr int NN = vamp::FFN_NODES, NPIX = 64 * TPIX;
        __shared__ double ell[NN][NPIX];
        __shared__ double w2s[NPIX], w2ds[NPIX], part[TPIX][2];
        const int p = (int)threadIdx.x;
        const double tp = (x[g] - mid) / half;
        double c[NN], den = 0.0;
        int hit = -1;
#pragma unroll
        for (int n = 0; n < NN; ++n) {
            const double tn = FF_M[FF_MAT + n], wn = sqrt((1.0 - tn) * (1.0 + tn)), diff = tp - tn;
            if (diff == 0.0) hit = n;
            c[n] = ((n & 1) ? -wn : wn) / diff;
            den += c[n];
        }
#pragma unroll
        for (int n = 0; n < NN; ++n) ell[n][p] = hit < 0 ? c[n] / den : (n == hit ? 1.0 : 0.0);
        const double w2 = wt[g] * wt[g], d = f[g] - 1.0, w2d = w2 * d;
        w2s[p] = w2;
        w2ds[p] = w2d;
        __syncthreads();
        double* mt = mom + (g0 >> 8) * vamp::FFN_TILE;
        const int n = p >> 4, m = p & (NN - 1);
        double qa[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sa[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < NPIX; i += 8) {
#pragma unroll
            for (int k = 0; k < 8; ++k) qa[k] = fma(w2s[i + k], ell[n][i + k] * ell[m][i + k], qa[k]);
        }
        mt[vamp::FFN_Q + p] = ((qa[0] + qa[1]) + (qa[2] + qa[3])) + ((qa[4] + qa[5]) + (qa[6] + qa[7]));
        if (p < NN) {
            for (int i = 0; i < NPIX; i += 8) {
#pragma unroll
                for (int k = 0; k < 8; ++k) sa[k] = fma(w2ds[i + k], ell[p][i + k], sa[k]);
            }
            mt[vamp::FFN_S + p] = ((sa[0] + sa[1]) + (sa[2] + sa[3])) + ((sa[4] + sa[5]) + (sa[6] + sa[7]));
        }
        const double cw = wave_sum<64>(w2d * d), qw = wave_sum<64>(w2);
        if ((p & 63) == 0) {
            part[p >> 6][0] = qw;
            part[p >> 6][1] = cw;
        }
        __syncthreads();
        if (p == 0) {
            const double q0 = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
            const double C0 = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
            mt[vamp::FFN_C0] = C0;
            mt[vamp::FFN_RC] = sqrt(C0);
            mt[vamp::FFN_RQ] = sqrt(q0);
        }
        if (p > vamp::FFN_RQ - vamp::FFN_S && p < vamp::FFN_TILE - vamp::FFN_S) mt[vamp::FFN_S + p] = 0.0;      // the padding
    }
#elif VAMP_TILE_MOMENTS
    // data moments of the tile (ff_moments.hpp): wavefront t holds quarter q, one pixel per lane; every sum in the one
    // order of wave_sum's tree, the powers of u by repeated multiplication
    if constexpr (!F32) {
        __shared__ double part[TPIX][2];
        double* mt = mom + (g0 >> 8) * vamp::FFM_TILE;
        const int lane = (int)threadIdx.x & 63;
        const double w2 = wt[g] * wt[g], d = f[g] - 1.0, w2d = w2 * d;
        double pw = 1.0;
        for (int n = 0; n < vamp::FFM_NQ; ++n) {
            const double sq = wave_sum<64>(w2 * pw);
            if (lane == 0) mt[q * vamp::FFM_QROW + n] = sq;
            if (n == 0 && lane == 0) part[q][0] = sq;
            if (n < vamp::FFM_NS) {
                const double ss = wave_sum<64>(w2d * pw);
                if (lane == 0) mt[vamp::FFM_S + q * vamp::FFM_NS + n] = ss;
            }
            pw *= ug;
        }
        const double c0 = wave_sum<64>(w2d * d);
        if (lane == 0) part[q][1] = c0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double q0 = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
            const double C0 = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
            mt[vamp::FFM_C0] = C0;
            mt[vamp::FFM_RC] = sqrt(C0);
            mt[vamp::FFM_RQ] = sqrt(q0);
            mt[3 * vamp::FFM_QROW + vamp::FFM_NQ] = 0.0;
        }
    }
#endif
}

// Sum over the walker's pixels of ((f - m) w)^2, on every lane.  One walker per wavefront (LPW = 64):
// full tiles are dealt round-robin into PARTS classes, each class is summed over its tiles and
// over the wave, and the class sums are added in class order -- by this wavefront (SPLIT = false)
// or through `red` by the PARTS wavefronts of the workgroup (SPLIT = true, `part` = this wave's
// class): the same order of additions either way.  The tail (pixels beyond the last full tile) belongs to class 0.
template <bool F32, int MODE, class PK, bool TAB = use_tables<F32, MODE, PK>()>
__device__ __forceinline__ void sweep_class(const RegionDev& R, const typename PK::Lds& L, TileScratch& Sx, const double* __restrict__ dct,
                                            const PixPtrs& px, int lane, int base0, int full, int stride, bool tail, double& chi,
                                            const double* tab) {
    constexpr int TPIX = pixels_per_lane<PK>();      // (shadows the global: packed shapes may hold fewer pixels per lane)
    if constexpr (F32) {
        const float* x = px.xf + R.pix_off; const float* f = px.ff + R.pix_off; const float* wt = px.wtf + R.pix_off;
        if constexpr (VAMP_FARFIELD && PK::FF && MODE != VAMP_GAUSS3 && TPIX == 4)
            sweep_range_f32_ff<MODE, PK, use_tables32<F32, MODE, PK>()>(R, L, Sx, dct, x, f, wt, px.uf + R.pix_off, px.geo + (R.pix_off >> 8),
                                                                        lane, base0, full, stride, chi, reinterpret_cast<const float*>(tab));
        else if (TPIX > 1) sweep_range_f32<MODE, PK, TPIX>(R, L, x, f, wt, lane, base0, full, stride, chi);
        if constexpr (PK::TAIL || TPIX == 1)
            if (tail) {
                const int from = TPIX > 1 ? full : 0;
                if constexpr (!PK::FF && TPIX > 1) {
                    // short regions are all "tail": one iteration with just enough pixels per lane (1..TPIX
                    // independent evaluation chains, all pixel loads in flight together) instead of up
                    // to TPIX dependent one-pixel rounds
                    const int nt = (R.P - from + PK::LPW - 1) / PK::LPW;
                    if constexpr (TPIX >= 4) { if (nt == 4) sweep_range_f32<MODE, PK, 4>(R, L, x, f, wt, lane, from, from + 1, 1 << 28, chi); }
                    if constexpr (TPIX >= 3) { if (nt == 3) sweep_range_f32<MODE, PK, 3>(R, L, x, f, wt, lane, from, from + 1, 1 << 28, chi); }
                    if (nt == 2) sweep_range_f32<MODE, PK, 2>(R, L, x, f, wt, lane, from, from + 1, 1 << 28, chi);
                    else if (nt == 1) sweep_range_f32<MODE, PK, 1>(R, L, x, f, wt, lane, from, from + 1, 1 << 28, chi);
                } else {
                    sweep_range_f32<MODE, PK, 1>(R, L, x, f, wt, lane, from, R.P, PK::LPW, chi);
                }
            }
    } else {
        const double* x = px.x + R.pix_off; const double* f = px.f + R.pix_off; const double* wt = px.wt + R.pix_off;
        if constexpr (VAMP_FARFIELD && PK::FF && MODE != VAMP_GAUSS3 && TPIX == 4) {
            // a tile starts at a multiple of 256 pixels of its region, so tile `base` is slot (pix_off >> 8) + (base >> 8)
            const double* ut = px.u + R.pix_off;
            const double2* geo = px.geo + (R.pix_off >> 8);
            const double* mom = VAMP_TILE_MOMENTS ? px.mom + (R.pix_off >> 8) * MOM_TILE : nullptr;
            // what stage_lines left in the parameter block: the mask of the lines far wider than a tile (none on a
            // converged ensemble) and, above it, the walker's guard bits (ff_guard_bits)
            const int flags = __builtin_amdgcn_readfirstlane((int)(__double_as_longlong(L.theta[4 * PK::KCAP + 2]) & 0x3ffff));
            const bool guard = (flags >> 16) != 0;
            if constexpr (VAMP_WIDE_NODES && TAB) {
                const unsigned long long wide_all = (unsigned long long)(flags & 0xffff);
                if (VAMP_MID_NODES || wide_all) {
                    if (guard) sweep_range_ff_any<MODE, PK, TAB, true, true>(R, L, Sx, dct, x, f, wt, ut, geo, lane, base0, full, stride, chi, tab, wide_all, mom);
                    else sweep_range_ff_any<MODE, PK, TAB, true, false, true>(R, L, Sx, dct, x, f, wt, ut, geo, lane, base0, full, stride, chi, tab, wide_all, mom);
                } else {
                    if (guard) sweep_range_ff_any<MODE, PK, TAB, false, true>(R, L, Sx, dct, x, f, wt, ut, geo, lane, base0, full, stride, chi, tab, 0ull, mom);
                    else sweep_range_ff_any<MODE, PK, TAB, false, false, true>(R, L, Sx, dct, x, f, wt, ut, geo, lane, base0, full, stride, chi, tab, 0ull, mom);
                }
            } else {
                if (guard) sweep_range_ff_any<MODE, PK, TAB, false, true>(R, L, Sx, dct, x, f, wt, ut, geo, lane, base0, full, stride, chi, tab, 0ull, mom);
                else sweep_range_ff_any<MODE, PK, TAB, false, false, true>(R, L, Sx, dct, x, f, wt, ut, geo, lane, base0, full, stride, chi, tab, 0ull, mom);
            }
        } else if (TPIX > 1) sweep_range<MODE, PK, TPIX, TAB>(R, L, x, f, wt, lane, base0, full, stride, chi, tab);
        if constexpr (PK::TAIL || TPIX == 1)
            if (tail) {
                const int from = TPIX > 1 ? full : 0;
                if constexpr (!PK::FF && TPIX > 1) {
                    const int nt = (R.P - from + PK::LPW - 1) / PK::LPW;      // see the fp32 branch
                    if constexpr (TPIX >= 4) { if (nt == 4) sweep_range<MODE, PK, 4, TAB>(R, L, x, f, wt, lane, from, from + 1, 1 << 28, chi, tab); }
                    if constexpr (TPIX >= 3) { if (nt == 3) sweep_range<MODE, PK, 3, TAB>(R, L, x, f, wt, lane, from, from + 1, 1 << 28, chi, tab); }
                    if (nt == 2) sweep_range<MODE, PK, 2, TAB>(R, L, x, f, wt, lane, from, from + 1, 1 << 28, chi, tab);
                    else if (nt == 1) sweep_range<MODE, PK, 1, TAB>(R, L, x, f, wt, lane, from, from + 1, 1 << 28, chi, tab);
                } else {
                    sweep_range<MODE, PK, 1, TAB>(R, L, x, f, wt, lane, from, R.P, PK::LPW, chi, tab);
                }
            }
    }
}

// ---- blends: tables of a few lines at a time, optical depths in registers across the passes -------
// T pixels per lane (base + 64 t + lane) of lines k0 .. k0 + kn - 1, whose tables sit in `tab`
template <int MODE, class PK, int T>
__device__ __forceinline__ void blend_chunk(const RegionDev& R, const typename PK::Lds& L, const double* __restrict__ x, int lane,
                                            int base, int k0, int kn, const double* tab, double (&tau)[4]) {
    double xi[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int i = base + 64 * t + lane;
        xi[t] = x[i < R.P ? i : R.P - 1];
    }
    for (int kk = 0; kk < kn; ++kk) {
        const LineRec ln = L.line[k0 + kk];
        double X[T], H[T];
#pragma unroll
        for (int t = 0; t < T; ++t) X[t] = fabs(xi[t] - ln.c) * ln.s;
        tile_voigt<T, true>(ln, L.dtab[k0 + kk], X, H, tab + kk * vamp::TAB_LINE);
#pragma unroll
        for (int t = 0; t < T; ++t) tau[t] = fma(ln.amp, H[t], tau[t]);
    }
}
template <int MODE, class PK>
__device__ __forceinline__ void blend_chunk_n(const RegionDev& R, const typename PK::Lds& L, const double* __restrict__ x, int lane,
                                              int base, int tn, int k0, int kn, const double* tab, double (&tau)[4]) {
    if (tn >= 4) blend_chunk<MODE, PK, 4>(R, L, x, lane, base, k0, kn, tab, tau);
    else if (tn == 3) blend_chunk<MODE, PK, 3>(R, L, x, lane, base, k0, kn, tab, tau);
    else if (tn == 2) blend_chunk<MODE, PK, 2>(R, L, x, lane, base, k0, kn, tab, tau);
    else if (tn == 1) blend_chunk<MODE, PK, 1>(R, L, x, lane, base, k0, kn, tab, tau);
}
constexpr int BLEND_MAX_PIXELS = 512;     // two chunks of up to 4 pixels per lane
template <int MODE, class PK>
__device__ __forceinline__ double sweep_blend_passes(const RegionDev& R, const typename PK::Lds& L, const PixPtrs& px, int lane,
                                                     double* tab) {
    static_assert(PK::WPB == 1 && PK::LPW == 64, "one wavefront per walker");
    constexpr int LP = PK::LINES_PER_PASS;
    const double* __restrict__ x = px.x + R.pix_off;
    const double* __restrict__ f = px.f + R.pix_off;
    const double* __restrict__ wt = px.wt + R.pix_off;
    const int P = R.P, K = R.K;
    const int nt = (P + 63) >> 6;                  // pixels per lane, <= 8
    const int tn0 = nt < 4 ? nt : 4, tn1 = nt - tn0;
    double tau0[4] = {0.0, 0.0, 0.0, 0.0}, tau1[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += LP) {
        const int kn = K - k0 < LP ? K - k0 : LP;
        // the tables of this pass: one (line, interval) pair per lane and round
        for (int e = lane; e < kn * vamp::TAB_NI; e += 64) {
            const int kk = e / vamp::TAB_NI, i = e % vamp::TAB_NI, k = k0 + kk;
            vamp::taylor_table_row(i, L.line[k].y, L.dtab[k], L.line[k].pole, L.line[k].hy, tab + kk * vamp::TAB_LINE + i * vamp::TAB_NT);
        }
        group_barrier<PK>();
        blend_chunk_n<MODE, PK>(R, L, x, lane, 0, tn0, k0, kn, tab, tau0);
        if (tn1 > 0) blend_chunk_n<MODE, PK>(R, L, x, lane, 256, tn1, k0, kn, tab, tau1);
        group_barrier<PK>();                        // the next pass overwrites the tables
    }
    double chi = 0.0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 256 * c + 64 * t + lane;
            if (64 * (4 * c + t) < P) {             // wave-uniform: this pixel slot exists
                const int idx = i < P ? i : P - 1;
                const double m = vamp::exp_taylor(-(c == 0 ? tau0[t] : tau1[t]));
                const double r = (f[idx] - m) * wt[idx];
                chi += i < P ? r * r : 0.0;
            }
        }
    }
    return wave_sum<64>(chi);
}

// fp32 blends: rows of every line built once (one (line, interval) pair per lane and round), then ONE sweep of the
// region's <= 512 pixels, 1..4 per lane and chunk, lines innermost: W4 regions I / II in the wings, a table look-up
// in the cores (tile_w4_tab)
template <int MODE, class PK, int T>
__device__ __forceinline__ void blend32_chunk(const RegionDev& R, const typename PK::Lds& L, const float* __restrict__ x,
                                              const float* __restrict__ f, const float* __restrict__ wt, int lane, int base,
                                              const float* tab32, double& chi) {
    float xi[T], tau[T];
    int idx[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int i = base + 64 * t + lane;
        idx[t] = i < R.P ? i : R.P - 1;
        xi[t] = x[idx[t]];
        tau[t] = 0.0f;
    }
    for (int k = 0; k < R.K; ++k) {
        const float c = L.linef[k][0], sc = L.linef[k][1], y = L.linef[k][2], a = L.linef[k][3];
        float X[T], H[T];
#pragma unroll
        for (int t = 0; t < T; ++t) X[t] = fabsf(xi[t] - c) * sc;
        tile_w4_tab<T>(y, X, H, tab32 + k * vamp::TAB32_LINE);
#pragma unroll
        for (int t = 0; t < T; ++t) tau[t] = fmaf(a, H[t], tau[t]);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float m = __expf(-tau[t]);
        const float r = (f[idx[t]] - m) * wt[idx[t]];
        chi += (base + 64 * t + lane) < R.P ? (double)r * (double)r : 0.0;
    }
}
template <int MODE, class PK>
__device__ __forceinline__ double sweep_blend32(const RegionDev& R, const typename PK::Lds& L, const PixPtrs& px, int lane, float* tab32) {
    static_assert(PK::WPB == 1 && PK::LPW == 64, "one wavefront per walker");
    const float* __restrict__ x = px.xf + R.pix_off;
    const float* __restrict__ f = px.ff + R.pix_off;
    const float* __restrict__ wt = px.wtf + R.pix_off;
    for (int e = lane; e < R.K * vamp::TAB_NI; e += 64) {
        const int k = e / vamp::TAB_NI, i = e % vamp::TAB_NI;
        vamp::taylor_table_row32(i, L.line[k].y, L.dtab[k], L.line[k].pole, L.line[k].hy, tab32 + k * vamp::TAB32_LINE + i * vamp::TAB32_NT);
    }
    group_barrier<PK>();
    double chi = 0.0;
    for (int base = 0; base < R.P; base += 256) {
        const int nt = (R.P - base + 63) >> 6;
        if (nt >= 4) blend32_chunk<MODE, PK, 4>(R, L, x, f, wt, lane, base, tab32, chi);
        else if (nt == 3) blend32_chunk<MODE, PK, 3>(R, L, x, f, wt, lane, base, tab32, chi);
        else if (nt == 2) blend32_chunk<MODE, PK, 2>(R, L, x, f, wt, lane, base, tab32, chi);
        else blend32_chunk<MODE, PK, 1>(R, L, x, f, wt, lane, base, tab32, chi);
    }
    return wave_sum<64>(chi);
}

template <bool F32, int MODE, class PK = PackWide>
__device__ __forceinline__ double sweep_pixels(const RegionDev& R, const typename PK::Lds& L, TileScratch& Sx, const double* __restrict__ dct,
                                               const PixPtrs& px, int lane, int part, double* red, const double* tab) {
    constexpr int TILE = PK::LPW * pixels_per_lane<PK>();
    const int full = (R.P / TILE) * TILE;
    if constexpr (PK::SUBS > 1) {            // several walkers per wavefront: short regions, one pass
        double chi = 0.0;
        sweep_class<F32, MODE, PK>(R, L, Sx, dct, px, lane, 0, full, TILE, true, chi, tab);
        return wave_sum<PK::LPW>(chi);
    } else if constexpr (use_blend32<F32, MODE, PK>()) {
        if (R.P <= BLEND_MAX_PIXELS) return sweep_blend32<MODE, PK>(R, L, px, lane, reinterpret_cast<float*>(const_cast<double*>(tab)));
        double chi = 0.0;      // (longer than a blend: only when this shape is forced on a long region)
        sweep_class<F32, MODE, PK>(R, L, Sx, dct, px, lane, 0, full, TILE, true, chi, nullptr);
        return wave_sum<64>(chi);
    } else if constexpr (PK::LINES_PER_PASS > 0 && use_tables<F32, MODE, PK>()) {
        if (R.P <= BLEND_MAX_PIXELS) return sweep_blend_passes<MODE, PK>(R, L, px, lane, const_cast<double*>(tab));
        // longer than the registers hold (only when this shape is forced on a long region): every
        // line through the per-pixel evaluator, no tables
        double chi = 0.0;
        sweep_class<F32, MODE, PK, false>(R, L, Sx, dct, px, lane, 0, full, TILE, true, chi, nullptr);
        return wave_sum<64>(chi);
    } else if constexpr (PK::SPLIT && !PK::FF) {
        // a blend of a few hundred pixels: the group's wavefronts take contiguous shares of the region
        // (whole 16-pixel runs), each swept as full tiles + one iteration of 1..4 pixels per lane
        const int share = ((R.P + PK::WPB - 1) / PK::WPB + 15) & ~15;
        const int lo = part * share;
        RegionDev Rs = R;
        Rs.P = lo + share < R.P ? lo + share : R.P;           // this wave's pixels end here
        double chi = 0.0;
        if (lo < Rs.P)
            sweep_class<F32, MODE, PK>(Rs, L, Sx, dct, px, lane, lo, lo + ((Rs.P - lo) / TILE) * TILE, TILE, true, chi, tab);
        chi = wave_sum<64>(chi);
        if (lane == 0) red[part] = chi;
        group_barrier<PK>();
        double total = 0.0;
#pragma unroll
        for (int p = 0; p < PK::WPB; ++p) total += red[p];
        return total;
    } else if constexpr (PK::SPLIT) {
        double chi = 0.0;
        sweep_class<F32, MODE, PK>(R, L, Sx, dct, px, lane, part * TILE, full, PARTS * TILE, part == 0, chi, tab);
        chi = wave_sum<64>(chi);
        if (lane == 0) red[part] = chi;
        __syncthreads();
        double total = 0.0;
#pragma unroll
        for (int p = 0; p < PARTS; ++p) total += red[p];
        return total;
    } else {
        double total = 0.0;
        for (int p = 0; p < PARTS; ++p) {
            double chi = 0.0;
            sweep_class<F32, MODE, PK>(R, L, Sx, dct, px, lane, p * TILE, full, PARTS * TILE, p == 0, chi, tab);
            total += wave_sum<64>(chi);
        }
        return total;
    }
}

// log-likelihood from the reduced sum (both forms of SURVEY Appendix A)
template <class LDS>
__device__ __forceinline__ double loglike_from_sum(const RegionDev& R, const LDS& L, double ssum) {
    if (R.sample_sd) {
        const double sd = L.theta[R.D - 1];
        const double t = 1.0 / (sd * sd);
        return (double)R.P * 0.5 * log(t / (2.0 * vamp::PI)) - 0.5 * t * ssum;   // vpfits.py:39,341
    }
    return -0.5 * ssum + R.norm_const;                                            // vpfits.py:118
}

// log-posterior of the walker whose parameters sit in L.theta; `lane` = lane inside the walker's
// group.  Groups of one wave may leave early independently: everything below communicates only
// inside a group (xor shuffles with offsets < LPW, group_any votes) or through __any, which ignores inactive lanes.
template <bool F32, int MODE, class PK = PackWide>
__device__ __forceinline__ double wave_lnprob(const RegionDev& R, typename PK::Lds& L, TileScratch& Sx, const double* dct,
                                              const PixPtrs& px, int lane, double* chi_out, int part, double* red, double* tab) {
    constexpr bool FFG = VAMP_FARFIELD && PK::FF && !F32 && MODE != VAMP_GAUSS3 && pixels_per_lane<PK>() == 4;   // sweep_class reads the bits
    const double lp = stage_lines<MODE, PK, use_tables<F32, MODE, PK>() && PK::LINES_PER_PASS == 0, use_tables32<F32, MODE, PK>(),
                                  use_blend32<F32, MODE, PK>(), FFG>(R, L, lane, F32, part, tab, FFG ? px.x + R.pix_off : nullptr);
    VAMP_STAMP(3);
    if (!(lp > NEG_INF) || lp != lp) {       // outside the prior (or NaN): skip the sweep
        if (chi_out) *chi_out = __builtin_nan("");
        return NEG_INF;
    }
#ifdef VAMP_SKIP_SWEEP    // timing-only builds (tools/variants.py)
    const double ssum = L.line[0].y + L.theta[lane & 31] + (tab ? tab[lane] : 0.0);
#else
    const double ssum = sweep_pixels<F32, MODE, PK>(R, L, Sx, dct, px, lane, part, red, tab);
#endif
    VAMP_STAMP(4);
    if (chi_out) *chi_out = ssum;
    double v = lp + loglike_from_sum(R, L, ssum);
    if (v != v) v = NEG_INF;                 // NaN -> -inf (emcee convention)
    return v;
}

// ---------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------
template <bool F32, int MODE, class PK>
__global__ __launch_bounds__(PK::THREADS, (min_waves<F32, PK>())) void k_lnprob(const RegionDev* __restrict__ regions, int region, PixPtrs px,
                                                  long long W, const double* __restrict__ theta,
                                                  double* __restrict__ lnprob, double* __restrict__ chi2,
                                                  const int* __restrict__ region_list) {
    // region < 0: several regions in one launch (blockIdx.y indexes region_list, or the regions
    // themselves when it is null); theta holds the regions' [W, D_r] blocks one after the other
    // (block r starts at W * d_before(r)), lnprob / chi2 are [n_regions, W]
    const bool all = region < 0;
    if (all) region = region_list ? region_list[blockIdx.y] : (int)blockIdx.y;
    __shared__ typename PK::Lds lds[PK::SPLIT ? 1 : PK::WPB * PK::SUBS];
    __shared__ TileScratch scr[PK::FF ? PK::WPB : 1];
    __shared__ alignas(16) double dct[PK::FF ? ff_table_doubles<F32>() : 1];
    __shared__ double red[PARTS];
    __shared__ LineTables<table_doubles<F32, MODE, PK>()> tabs[PK::SPLIT ? 1 : PK::WPB];
    if constexpr (PK::FF) ff_fill_table<F32>(dct);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sub = lane / PK::LPW, l = lane % PK::LPW;
    const long long w = PK::SPLIT ? (long long)blockIdx.x : ((long long)blockIdx.x * PK::WPB + wave) * PK::SUBS + sub;
    if (w >= W) return;
    const RegionDev R = regions[region];
    if (all) {
        theta += W * R.d_before;
        lnprob += (long long)region * W;
        if (chi2) chi2 += (long long)region * W;
    }
    typename PK::Lds& L = lds[PK::SPLIT ? 0 : wave * PK::SUBS + sub];
    if (!PK::SPLIT || wave == 0)
        for (int d = l; d < R.D; d += PK::LPW) L.theta[d] = theta[w * R.D + d];
    group_barrier<PK>();
    double chi;
    const double v = wave_lnprob<F32, MODE, PK>(R, L, scr[PK::FF ? wave : 0], dct, px, l, &chi, wave, red,
                                                tabs[PK::SPLIT ? 0 : wave].a);
    if (PK::SPLIT && wave != 0) return;
    if (l == 0) {
        lnprob[w] = v;
        if (chi2) chi2[w] = chi;
    }
}

// Test hook (vampdbg_node_sums): the node stage of every full tile of one region for one parameter vector, through the
// device functions the fp64 far-field loop calls -- the classification and ff_node_pass for the full batches of a
// wavefront's tiles, ff_classify_batch / ff_wide_nodes / ff_node_sums for what is left -- in the workgroup-per-walker
// shape (wavefront j sweeps tile class j).  nodes[tile][16]; sets[first tile of a full batch][5] = {far, n6, n4, n3, wide}.
template <int MODE>
__global__ __launch_bounds__(PackSplit::THREADS) void k_dbg_node_sums(const RegionDev* __restrict__ regions, int region, PixPtrs px,
                                                                      const double* __restrict__ theta, double* __restrict__ nodes,
                                                                      unsigned* __restrict__ sets_out, bool adj_) {
    using PK = PackSplit;
    const bool adj = VAMP_DEAL_ADJ && adj_;
    __shared__ typename PK::Lds lds[1];
    __shared__ TileScratch scr[PK::WPB];
    __shared__ alignas(16) double dct[ff_table_doubles<false>()];
    __shared__ LineTables<table_doubles<false, MODE, PK>()> tabs[1];
    ff_fill_table<false>(dct);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const RegionDev R = regions[region];
    typename PK::Lds& L = lds[0];
    if (wave == 0)
        for (int d = lane; d < R.D; d += 64) L.theta[d] = theta[d];
    group_barrier<PK>();
    const double lp = stage_lines<MODE, PK, true, false, false, true>(R, L, lane, false, wave, tabs[0].a, px.x + R.pix_off);
    if (!(lp > NEG_INF)) return;
    TileScratch& Sx = scr[wave];
    const double* tab = tabs[0].a;
    const double2* geo = px.geo + (R.pix_off >> 8);
    const int flags = __builtin_amdgcn_readfirstlane((int)(__double_as_longlong(L.theta[4 * PK::KCAP + 2]) & 0x3ffff));
    const bool guard = (flags >> 16) != 0;
    const unsigned wide_all = (unsigned)(flags & 0xffff);
    constexpr int TILE = 64 * TPIX;
    const int K = R.K, base1 = (R.P / TILE) * TILE, stride = PARTS * TILE;
    const int base0 = __builtin_amdgcn_readfirstlane(wave * TILE);
    int bfull = base0, brest = base0;
#if VAMP_NODE_PASS_ON
    // adj: the batches of sweep_range_ff_np with VAMP_DEAL_ADJ (four adjacent tiles); else a class's tiles four at a time
    const int ntile = base0 < base1 ? (base1 - base0 + stride - 1) / stride : 0;
    const int tstride = adj ? TILE : stride, bstep = FF_BATCH * stride;
    bfull = __builtin_amdgcn_readfirstlane(adj ? (base1 / bstep) * bstep : base0 + (ntile / FF_BATCH) * bstep);
    brest = adj ? bfull + base0 : bfull;
    for (int batch = adj ? FF_BATCH * base0 : base0; batch < bfull; batch += bstep) {
        unsigned long long farmasks, widemasks, zonemasks;
        NodeSets sets;
        double mid, half;
        ff_classify_batch_np<true, true>(L, geo, K, lane, batch, tstride, wide_all, farmasks, widemasks, zonemasks, sets, mid, half);
        double fs0 = 0.0;
#if VAMP_SUPER_ON
        if (adj && !guard && wide_all == 0u) fs0 = ff_super_batch(L, Sx, dct, geo, K, lane, batch, tstride, mid, half, farmasks, sets);
#endif
        const double fs = guard ? ff_node_pass<true, true>(L, dct, tab, lane, mid, half, farmasks, widemasks, sets)
                                : ff_node_pass<true, false>(L, dct, tab, lane, mid, half, farmasks, widemasks, sets, fs0);
        nodes[((batch + (lane >> 4) * tstride) >> 8) * FF_NODES + (lane & (FF_NODES - 1))] = fs;
        if (lane == 0) {
            unsigned* so = sets_out + (batch >> 8) * 5;
            so[0] = sets.far, so[1] = sets.n6, so[2] = sets.n4, so[3] = sets.n3, so[4] = sets.wide;
        }
    }
#endif
    for (int batch = brest; batch < base1; batch += FF_BATCH * stride) {
        unsigned long long farmasks, widemasks, zonemasks;
        ff_classify_batch<true, false, true>(L, Sx, geo, K, lane, batch, base1, stride, wide_all, farmasks, widemasks, zonemasks);
        for (int j = 0; j < FF_BATCH; ++j, farmasks >>= KMAX, widemasks >>= KMAX) {
            const int base = batch + j * stride;
            if (base >= base1) break;
            const double2 tg = geo[base >> 8];
            const double mid = tg.x, half = fabs(tg.y);
            const int nfar = __builtin_popcount((unsigned)farmasks & 0xffffu), nwide = __builtin_popcount((unsigned)widemasks & 0xffffu);
            const double fs_wide = nwide > 0 ? ff_wide_nodes<typename PK::Lds>(L, Sx.widelist[j], dct, tab, lane, nwide, mid, half) : 0.0;
            const double fs = guard ? ff_node_sums<typename PK::Lds, true>(L, Sx.farlist[j], dct, lane, nfar, mid, half, fs_wide)
                                    : ff_node_sums<typename PK::Lds, false>(L, Sx.farlist[j], dct, lane, nfar, mid, half, fs_wide);
            if (lane < FF_NODES) nodes[(base >> 8) * FF_NODES + lane] = fs;
        }
        __builtin_amdgcn_wave_barrier();      // (the next batch's lists overwrite these)
    }
}

// ---- MAP search on the device (row a9: VPfit.map_estimate / the MAP calls of find_bic, vpfits.py:352-358, 426) -------
// One workgroup per region runs the WHOLE Nelder-Mead search of that region -- scipy fmin's rules as restated in
// csrc/map_search.hpp, with the arithmetic of a simplex update shared with it (vamp::nm_*) -- in one launch: the
// host-driven form of the same search costs one launch + one stream synchronisation per ITERATION (~55 us each,
// ~60 000 per q1422 fit).  The workgroup has the shape k_lnprob runs for the region's launch class, so a point's
// objective has the bits vamp_lnprob gives it; its SLOTS walker slots evaluate the candidates of an iteration
// together (reflection, expansion and both contractions when SLOTS >= 4 -- the speculative form of the host
// search -- otherwise reflection first and the one point fmin asks for next).  The simplex lives in LDS
// up to D = 33, else in global scratch ((D + 1) x D doubles per region, L2-resident), values / order / centroid in LDS; the vertices are never
// moved, `ord` holds their order.  Regions are independent: no inter-workgroup communication.
constexpr int NM_INIT = 0, NM_CAND = 1, NM_CAND2 = 2, NM_SHRINK = 3;
constexpr int NM_LDS_DOUBLES = 34 * 33 + 2;      // simplices up to this size live in LDS (9 KB)
struct MapLds {
    double xbar[DMAX], worst[DMAX];   // centroid of the N best vertices, the worst vertex
    double f[DMAX + 1];               // objective values, ascending
    int ord[DMAX + 1];                // ord[k] = row of the k-th best vertex
    double fv[16];                    // values of the points evaluated in this round, by slot
    double redx[WAVES_PER_BLOCK], redf[WAVES_PER_BLOCK];
    double f0;                        // value at the start point
};
template <bool F32, int MODE, class PK>
__global__ __launch_bounds__(PK::THREADS, (min_waves<F32, PK>())) void k_map_search(
    const RegionDev* __restrict__ regions, PixPtrs px, const int* __restrict__ region_list, const double* __restrict__ theta0,
    const unsigned char* __restrict__ active, long long maxiter, long long maxfun, double xtol, double ftol,
    double* __restrict__ scratch, double* __restrict__ theta_best, long long* __restrict__ iterations) {
    constexpr int SLOTS = PK::WALKERS_PER_BLOCK, NT = PK::THREADS;
    static_assert(SLOTS <= 16 && PK::WPB <= WAVES_PER_BLOCK, "MapLds::fv / redx");
    __shared__ typename PK::Lds lds[PK::SPLIT ? 1 : PK::WPB * PK::SUBS];
    __shared__ TileScratch scr[PK::FF ? PK::WPB : 1];
    __shared__ alignas(16) double dct[PK::FF ? ff_table_doubles<F32>() : 1];
    __shared__ double red[PARTS];
    __shared__ LineTables<table_doubles<F32, MODE, PK>()> tabs[PK::SPLIT ? 1 : PK::WPB];
    __shared__ MapLds M;
    if constexpr (PK::FF) ff_fill_table<F32>(dct);
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int sub = lane / PK::LPW, l = lane % PK::LPW;
    const int slot = PK::SPLIT ? 0 : wave * PK::SUBS + sub;
    const int region = region_list ? region_list[blockIdx.x] : (int)blockIdx.x;
    const RegionDev R = regions[region];
    const int N = R.D;
    theta0 += R.d_before;
    theta_best += R.d_before;
    if (active && !active[region]) {            // not searched: returned unchanged (uniform over the workgroup)
        for (int d = tid; d < N; d += NT) theta_best[d] = theta0[d];
        if (tid == 0) iterations[region] = 0;
        return;
    }
    // rows of N doubles: the N + 1 vertices -- in LDS up to N = 33 (8 Voigt lines + sd), else in global scratch
    __shared__ double sim_lds[NM_LDS_DOUBLES];
    double* sim = (N + 1) * N <= NM_LDS_DOUBLES ? sim_lds : scratch + R.sim_off;
    typename PK::Lds& L = lds[slot];
    // start simplex: the start point and one vertex per coordinate (vamp::nm_start_coordinate)
    for (int e = tid; e < (N + 1) * N; e += NT) {
        const int k = e / N, d = e - k * N;
        const double v = theta0[d];
        sim[e] = (k >= 1 && d == k - 1) ? vamp::nm_start_coordinate(v) : v;
    }
    for (int k = tid; k <= N; k += NT) M.ord[k] = k;
    const long long fun_cap = maxfun > 0 ? maxfun : 200ll * N;     // scipy's default: 200 evaluations per dimension
    int phase = NM_INIT, base = 0, need = 0;
    long long it = 0, calls = 0;
    for (;;) {
        __syncthreads();            // the simplex (global), the values and the order (LDS) as the last round left them
        int n_pts = 0;
        if (phase == NM_CAND) {
            // fmin's limits, then its stopping test: max |x_k - x_0| <= xtol and max |f_0 - f_k| <= ftol
            if (calls >= fun_cap || it + 1 >= maxiter) break;         // fmin counts iterations from 1
            double mx = 0.0, mf = 0.0;
            for (int d = tid; d < N; d += NT) {
                const double r0 = sim[(long long)M.ord[0] * N + d];
                double sum = 0.0 + r0;          // (the host search starts its sum at +0)
                for (int k = 1; k < N; ++k) {
                    const double v = sim[(long long)M.ord[k] * N + d];
                    sum += v;
                    mx = fmax(mx, fabs(v - r0));
                }
                const double vw = sim[(long long)M.ord[N] * N + d];
                mx = fmax(mx, fabs(vw - r0));
                M.xbar[d] = sum / (double)N;
                M.worst[d] = vw;
            }
            for (int k = 1 + tid; k <= N; k += NT) mf = fmax(mf, fabs(M.f[0] - M.f[k]));
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                mx = fmax(mx, __shfl_xor(mx, off, 64));
                mf = fmax(mf, __shfl_xor(mf, off, 64));
            }
            if (lane == 0) { M.redx[wave] = mx; M.redf[wave] = mf; }
            __syncthreads();
            mx = M.redx[0]; mf = M.redf[0];
#pragma unroll
            for (int w = 1; w < PK::WPB; ++w) { mx = fmax(mx, M.redx[w]); mf = fmax(mf, M.redf[w]); }
            if (mx <= xtol && mf <= ftol) break;
            n_pts = SLOTS < 4 ? SLOTS : 4;
        } else if (phase == NM_CAND2) {
            n_pts = 1;
        } else {
            const int left = (phase == NM_INIT ? N + 1 : N) - base;
            n_pts = left < SLOTS ? left : SLOTS;
        }
        // this slot's point -> its parameter block in LDS, evaluated by the slot's lanes
        const bool mine = slot < n_pts;
        if (mine) {
            if (!PK::SPLIT || wave == 0) {
                if (phase == NM_CAND || phase == NM_CAND2) {
                    const int which = phase == NM_CAND ? slot : need;
                    for (int d = l; d < N; d += PK::LPW) L.theta[d] = vamp::nm_candidate(which, M.xbar[d], M.worst[d]);
                } else {
                    const double* row = sim + (long long)M.ord[(phase == NM_INIT ? 0 : 1) + base + slot] * N;
                    for (int d = l; d < N; d += PK::LPW) L.theta[d] = row[d];
                }
            }
            group_barrier<PK>();
            const double v = wave_lnprob<F32, MODE, PK>(R, L, scr[PK::FF ? wave : 0], dct, px, l, nullptr, wave, red,
                                                        tabs[PK::SPLIT ? 0 : wave].a);
            if (l == 0 && (!PK::SPLIT || wave == 0)) M.fv[slot] = vamp::nm_objective(v);
        }
        __syncthreads();
        // consume the round: every thread takes the same decisions from the same LDS values
        if (phase == NM_INIT || phase == NM_SHRINK) {
            const int first = (phase == NM_INIT ? 0 : 1) + base;
            if (tid < n_pts) M.f[first + tid] = M.fv[tid];
            base += n_pts;
            if (base < (phase == NM_INIT ? N + 1 : N)) continue;
            __syncthreads();
            if (phase == NM_INIT) calls = N + 1;
            else { calls += N; it += 1; }
            if (tid == 0) {
                if (phase == NM_INIT) M.f0 = M.f[0];
                for (int i = 1; i <= N; ++i) {              // insertion sort, stable: ties keep their order
                    const double fi = M.f[i];
                    const int oi = M.ord[i];
                    int j = i;
                    while (j > 0 && fi < M.f[j - 1]) { M.f[j] = M.f[j - 1]; M.ord[j] = M.ord[j - 1]; --j; }
                    M.f[j] = fi; M.ord[j] = oi;
                }
            }
            phase = NM_CAND;
            continue;
        }
        // NM_CAND / NM_CAND2: fmin's decision; a value this round did not hold is asked for (slots < 4)
        const int have = phase == NM_CAND ? n_pts : 0;           // candidates 0 .. have - 1 sit in fv[0 .. have)
        const double f_best = M.f[0], f_second = M.f[N - 1], f_worst = M.f[N];
        double fr;
        if (phase == NM_CAND) { fr = M.fv[0]; if (tid == 0) M.redx[0] = fr; }      // (kept for a second round)
        else fr = M.redx[0];
        int want;                               // the candidate whose value decides the update
        if (fr < f_best) want = 1;
        else if (fr < f_second) want = 0;
        else if (fr < f_worst) want = 2;
        else want = 3;
        double fw;
        if (want < have) fw = M.fv[want];
        else if (phase == NM_CAND2) fw = M.fv[0];
        else { phase = NM_CAND2; need = want; continue; }
        int take = -1;                          // candidate that replaces the worst vertex, or -1: shrink
        double ft = 0.0;
        calls += 1;
        if (want == 1) { calls += 1; if (fw < fr) { take = 1; ft = fw; } else { take = 0; ft = fr; } }
        else if (want == 0) { take = 0; ft = fr; }
        else if (want == 2) { calls += 1; if (fw <= fr) { take = 2; ft = fw; } }
        else { calls += 1; if (fw < f_worst) { take = 3; ft = fw; } }
        const int on = M.ord[N];                // row of the worst vertex
        __syncthreads();                        // (every thread has read fv / redx / f / ord before they change)
        if (take >= 0) {
            double* row = sim + (long long)on * N;
            for (int d = tid; d < N; d += NT) row[d] = vamp::nm_candidate(take, M.xbar[d], M.worst[d]);
            if (tid == 0) {                     // the new value finds its place among the N others (stable)
                int j = N;
                while (j > 0 && ft < M.f[j - 1]) { M.f[j] = M.f[j - 1]; M.ord[j] = M.ord[j - 1]; --j; }
                M.f[j] = ft; M.ord[j] = on;
            }
            it += 1;
            phase = NM_CAND;
        } else {
            for (int e = tid; e < N * N; e += NT) {
                const int k = 1 + e / N, d = e % N;
                double* row = sim + (long long)M.ord[k] * N;
                row[d] = vamp::nm_shrink(sim[(long long)M.ord[0] * N + d], row[d]);
            }
            phase = NM_SHRINK;
            base = 0;
        }
    }
    // the best vertex, unless it is worse than the start point
    const bool keep_start = M.f[0] > M.f0;
    const double* best = keep_start ? theta0 : sim + (long long)M.ord[0] * N;
    for (int d = tid; d < N; d += NT) theta_best[d] = best[d];
    if (tid == 0) iterations[region] = it;
}

// tau_k[P] and flux[P] for one parameter vector (one thread per pixel).  region < 0: every region in
// one launch (blockIdx.y = region): theta holds the regions' D_r-vectors one after the other,
// tau_comp the [K_r, P_r] blocks one after the other, flux_model is laid out like the pixels.
template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_model(const RegionDev* __restrict__ regions, int region, PixPtrs px,
                                                 const double* __restrict__ theta, double* __restrict__ tau_comp,
                                                 double* __restrict__ flux_model) {
    __shared__ WaveLds lds[WAVES_PER_BLOCK];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool all = region < 0;
    if (all) region = blockIdx.y;
    const RegionDev R = regions[region];
    if ((int)(blockIdx.x * BLOCK) >= R.P) return;          // (uniform per block: regions differ in length)
    if (all) {
        theta += R.d_before;
        if (tau_comp) tau_comp += R.tau_off;
        if (flux_model) flux_model += R.pix_off;
    }
    WaveLds& L = lds[wave];
    for (int d = lane; d < R.D; d += 64) L.theta[d] = theta[d];
    __builtin_amdgcn_wave_barrier();
    (void)stage_lines<MODE, PackXL>(R, L, lane, false, 0);
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= R.P) return;
    const double xi = px.x[R.pix_off + i];
    double tau = 0.0;
    for (int k = 0; k < R.K; ++k) {
        double tk;
        if constexpr (MODE == VAMP_GAUSS3) {
            const double u = (xi - L.line[k].c) * L.line[k].s;
            tk = L.line[k].amp * exp(-0.5 * (u * u));
        } else {
            const double X = fabs(xi - L.line[k].c) * L.line[k].s;
            tk = L.line[k].amp * vamp::voigt_Hs(X, L.line[k].y, L.dtab[k], L.line[k].pole, L.line[k].hy);
        }
        if (tau_comp) tau_comp[(long long)k * R.P + i] = tk;
        tau += tk;
    }
    if (flux_model) flux_model[i] = exp(-tau);
}

// staged per-line records of one parameter vector (test hook for the parameter maps)
template <int MODE>
__global__ __launch_bounds__(64) void k_line_records(const RegionDev* __restrict__ regions, int region,
                                                     const double* __restrict__ theta, double* __restrict__ rec,
                                                     double* __restrict__ lnprior) {
    __shared__ WaveLds lds[1];
    const int lane = threadIdx.x & 63;
    const RegionDev R = regions[region];
    WaveLds& L = lds[0];
    for (int d = lane; d < R.D; d += 64) L.theta[d] = theta[d];
    __builtin_amdgcn_wave_barrier();
    const double lp = stage_lines<MODE, PackXL>(R, L, lane, false, 0);
    if (lane < R.K) {
        rec[5 * lane + 0] = L.line[lane].c;
        rec[5 * lane + 1] = L.line[lane].s;
        rec[5 * lane + 2] = L.line[lane].y;
        rec[5 * lane + 3] = (MODE == VAMP_GAUSS3) ? L.line[lane].amp : L.line[lane].amp * SQRT_PI;   // oracle's tau scale
        rec[5 * lane + 4] = L.line[lane].pole;
    }
    if (lane == 0) *lnprior = lp;
}

template <bool F32>
__global__ __launch_bounds__(BLOCK) void k_wofz(long long n, const double* __restrict__ x, const double* __restrict__ y,
                                                double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (F32) {
        out[i] = (double)vamp::humlicek_w4_re(fminf(fabsf((float)x[i]), vamp::W4_XMAX), (float)y[i]);
    } else {
        double dtab[vamp::DTAB_N];
        for (int k = 0; k < vamp::DTAB_N; ++k) dtab[k] = vamp::core_dtab_entry(k, y[i]);
        out[i] = vamp::voigt_H(fabs(x[i]), y[i], dtab, vamp::core_pole_factor(y[i]), vamp::core_hy(y[i]));
    }
}

// ---- counter-based draws: Philox4x32-10, the keyed red/blue split, the draws of a mover (draws.hpp) ----
using vamp::MoveDraw; using vamp::draw_move;

struct SamplerDev {
    const RegionDev* regions;
    int n_regions;
    long long W;                 // walkers per region
    int split_block;
    double a;
    unsigned long long seed;
    double* X;                   // concatenated [W, D_r] blocks
    double* lnp;                 // [n_regions * W]
    long long* n_accept;         // [n_regions * W]
    long long slot_begin, slot_end;   // this ctx's share of the n_regions*W/2 active slots
    const int* region_list;      // this launch's regions (a launch class of the ctx), or nullptr = all, in order
    double* pack;                // walker-sharded runs: [slot - slot_begin][D + 1] = the mover's row and lnprob
                                 // after the accept step (what the other devices need), else nullptr
    int bpr, n_cls_regions;      // several regions: workgroups per region (0: workgroups do not align with regions) and the
                                 // regions of this launch, for the region -> XCD mapping of k_half_step
    int wpr;                     // packed shapes, several regions: wavefronts per region = ceil((W/2) / SUBS), so that every
                                 // wavefront lies inside one region whatever W is (the last one of a region may have idle
                                 // groups); 0: slots are dealt to wavefronts linearly (one region, or one walker per wavefront)
};

__host__ __device__ __forceinline__ int region_rng_id(const SamplerDev& S, int region) { return S.regions[region].rng_id; }

// Draws of a whole launch, one THREAD per mover.  A wavefront that serves one walker computes its
// draws on the scalar unit for free; packed four to a wavefront the same integer arithmetic runs
// on the vector unit with 4 distinct values in 64 lanes (~550 of ~1300 fixed instructions per
// wavefront, measured through profiles/r02_a_config3_pmc_summary.txt) -- so packed launches draw
// here, 64 distinct movers per instruction, and the half-step kernel reads the result.
__global__ __launch_bounds__(256) void k_draws(SamplerDev S, unsigned step, int half, long long n, int* __restrict__ ws,
                                               int* __restrict__ wc, double* __restrict__ z, double* __restrict__ logu,
                                               double* __restrict__ logz) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long halfW = S.W >> 1;
    const long long slot = i + S.slot_begin;
    const int ridx = (int)(slot / halfW);
    const int region = S.region_list ? S.region_list[ridx] : ridx;
    const MoveDraw d = draw_move(S, step, half, region, slot - (long long)ridx * halfW);
    ws[i] = (int)d.ws;
    wc[i] = (int)d.wc;
    z[i] = d.z;
    logu[i] = d.logu;
    logz[i] = log(d.z);
}

constexpr int DRAW_INLINE = 0, DRAW_HOST = 1, DRAW_PRE = 2;      // where a mover's draws come from (k_half_step)
#ifndef VAMP_UNIFORM_ACCEPT
#define VAMP_UNIFORM_ACCEPT 1
#endif
__device__ __forceinline__ double uniform_double(double v) {      // a wave-uniform value, moved to scalar registers
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// One mover of a half-step: proposal q = c - (c - s) z into the walker's parameter block in LDS, its log-posterior,
// the accept test and the state update.  `l` = lane inside the walker's group, `part` = the
// wavefront's index in a split group; pack_slot >= 0: the row this walker ends with also goes to the exchange buffer.
// Shared by k_half_step (one launch per half-step) and k_run_resident (the step loop inside the kernel): a walker
// follows the same arithmetic through either.
template <bool F32, int DRAWS, int MODE, class PK>
__device__ __forceinline__ void stretch_move(const SamplerDev& S, const RegionDev& R, typename PK::Lds& L, TileScratch& Sx,
                                             const double* dct, const PixPtrs& px, int l, int part, double* red, double* tab,
                                             long long ws, long long wc, double z, double logu, double logz, long long pack_slot) {
#ifdef VAMP_ROWS_CACHED    // timing-only builds: every row read hits a 64-row window (no HBM latency)
    double* Xs = S.X + R.theta_off + (ws & 63) * R.D;
    const double* Xc = S.X + R.theta_off + (wc & 63) * R.D;
    const long long wg = R.walker_off + (ws & 63);
#else
    double* Xs = S.X + R.theta_off + ws * R.D;
    const double* Xc = S.X + R.theta_off + wc * R.D;
    const long long wg = R.walker_off + ws;
#endif
    // the mover's current lnprob is requested together with the two rows: three random reads of a
    // state far larger than L2, one exposed round trip instead of two (it is needed only for the
    // accept test, and left there its miss is paid in full by the one or two waves a SIMD holds)
    VAMP_STAMP(1);
    double lnp_s = S.lnp[wg];
    if (!PK::SPLIT || part == 0)
        for (int d = l; d < R.D; d += PK::LPW) {
            const double c = Xc[d];
            L.theta[d] = c - (c - Xs[d]) * z;                 // q = c - (c - s) z
        }
    VAMP_STAMP(2);
#if VAMP_EARLY_LNP
    asm volatile("" : "+v"(lnp_s));                          // keep the read up here
#endif
    group_barrier<PK>();
    if constexpr (PK::LPW == 64 && VAMP_UNIFORM_ACCEPT) {
        // one walker per wavefront: the values the accept step needs after the sweep are the same in every lane -- hand
        // them to the scalar registers, where they do not compete with the sweep for the 128 vector registers of the
        // workgroup-per-walker shape (they were spilled around the sweep: 10 dwords per lane, 230 MB of scratch stores
        // per launch of the headline)
        lnp_s = uniform_double(lnp_s);
        logu = uniform_double(logu);
        z = uniform_double(z);
        logz = uniform_double(logz);
    }
    const double lnp_q = wave_lnprob<F32, MODE, PK>(R, L, Sx, dct, px, l, nullptr, part, red, tab);
    VAMP_STAMP(5);
    if (PK::SPLIT && part != 0) return;     // the group's first wave carries out the accept step
    if constexpr (DRAWS != DRAW_PRE) logz = log(z);
    const double diff = (double)(R.D - 1) * logz + lnp_q - lnp_s;
    const bool accept = logu < diff;                      // false for NaN
    if (pack_slot >= 0 && S.pack) {
        // active-colour exchange: the row this walker ends the half-step with, in slot order
        double* pk = S.pack + pack_slot * (long long)(R.D + 1);
        for (int d = l; d < R.D; d += PK::LPW) pk[d] = accept ? L.theta[d] : Xs[d];
        if (l == 0) pk[R.D] = accept ? lnp_q : lnp_s;
    }
    if (accept) {
        for (int d = l; d < R.D; d += PK::LPW) Xs[d] = L.theta[d];
        if (l == 0) {
            S.lnp[wg] = lnp_q;
            S.n_accept[wg] += 1;
        }
    }
    VAMP_STAMP(6);
}

// One half-step of the stretch move, one wavefront per active walker.
//   DRAWS = DRAW_INLINE: Philox in-kernel; DRAW_HOST: every draw supplied by the host for ONE region
//   (deterministic-parity hook); DRAW_PRE: read from the arrays k_draws filled for this launch.
// Wavefronts per SIMD are set per shape (Pack::MIN_WAVES): the tile code is latency-bound in places (LDS and
// scalar-cache round trips); the headline shape measured 4.29 / 3.46 / 3.28 ms at 2 / 3 / 4 of them
template <bool F32, int DRAWS, int MODE, class PK>
__global__ __launch_bounds__(PK::THREADS, (min_waves<F32, PK>())) void k_half_step(SamplerDev S, PixPtrs px, unsigned step, int half, int ext_region,
                                                     long long ext_n, const int* __restrict__ ext_active,
                                                     const int* __restrict__ ext_partner, const double* __restrict__ ext_z,
                                                     const double* __restrict__ ext_logu, const double* __restrict__ ext_logz) {
    constexpr bool EXT = DRAWS == DRAW_HOST;
    __shared__ typename PK::Lds lds[PK::SPLIT ? 1 : PK::WPB * PK::SUBS];
    __shared__ TileScratch scr[PK::FF ? PK::WPB : 1];
    __shared__ alignas(16) double dct[PK::FF ? ff_table_doubles<F32>() : 1];
    __shared__ double red[PARTS];
    __shared__ LineTables<table_doubles<F32, MODE, PK>()> tabs[PK::SPLIT ? 1 : PK::WPB];
    if constexpr (PK::FF) ff_fill_table<F32>(dct);
    const int lane = threadIdx.x & 63;
    // the wave index is the same in every lane: say so, and the draws below (Philox rounds, the
    // split bijection -- all integer) run on the scalar unit when a wave serves one walker
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane / PK::LPW, l = lane % PK::LPW;
    const long long halfW = S.W >> 1;
    // first walker of this wave (a split workgroup: the one walker all of its waves serve)
    // Workgroups are dealt round-robin to the eight XCDs (workgroup b runs on XCD b % 8), each with its own L2.  In a
    // context of several regions the movers of a region read rows of that region only, so a mapping that keeps a
    // region on ONE XCD (-DVAMP_XCD_MAP=1: region i of the launch on XCD i % 8, vamp::plan::xcd_map) fetches its state
    // into one L2 instead of up to eight.  MEASURED on q1422 (profiles/r04_d_xcd_mapping.txt): FETCH_SIZE per half-step
    // 782 -> 309 MB (TCC misses 11.8 M -> 5.0 M) as predicted -- and 3.64 ms against 3.37 per half-step in fp64, 1.84
    // against 1.71 in fp32: regions differ in cost (the 54 blends: 3 .. 8 lines over 96 .. 512 px, six or seven per
    // XCD), the round-robin deal balances them and the mapping does not; contiguous eighths of the launch per XCD
    // were worse still (4.13 ms).  These kernels are bound by instruction issue, not by the row gathers.  Off.
    // (One region -- the headline: every workgroup reads the same spectrum and random rows of one state: nothing to align.)
    long long b = blockIdx.x;
#if VAMP_XCD_MAP
    if (DRAWS != DRAW_HOST && S.bpr > 0) b = vamp::plan::xcd_map(b, S.n_cls_regions, S.bpr);   // (the last n % 8 regions keep their place)
#endif
    long long slot0 = PK::SPLIT ? b : (b * PK::WPB + wave) * PK::SUBS;
    if (PK::SUBS > 1 && DRAWS != DRAW_HOST && S.wpr > 0) {
        // several regions, several walkers per wavefront: wavefront g serves SUBS consecutive movers of region
        // g / wpr; the groups beyond the region's W/2 movers idle (below: slot0 + sub leaves the region's range)
        const long long g = b * PK::WPB + wave;
        const long long ri = g / S.wpr;
        slot0 = ri * halfW + (g - ri * S.wpr) * PK::SUBS;
        if (slot0 + sub >= (ri + 1) * halfW) return;
    }
    long long slot = slot0 + sub;
    int region;
    long long ws, wc;            // local walker ids (within the region) of mover and partner
    double z, logu, logz = 0.0;
    if constexpr (DRAWS == DRAW_HOST) {
        if (slot >= ext_n) return;
        region = ext_region;
        ws = ext_active[slot]; wc = ext_partner[slot]; z = ext_z[slot]; logu = ext_logu[slot];
    } else {
        const long long i = slot;                     // index inside this launch
        slot += S.slot_begin;
        if (slot >= S.slot_end) return;
        // every walker of a wave lies in one region (one region in all, or wavefronts dealt per region: S.wpr):
        // keep the region description in scalar registers
        const int ridx = __builtin_amdgcn_readfirstlane((int)((slot0 + S.slot_begin) / halfW));
        region = __builtin_amdgcn_readfirstlane(S.region_list ? S.region_list[ridx] : ridx);
        if constexpr (DRAWS == DRAW_PRE) {
            ws = ext_active[i]; wc = ext_partner[i]; z = ext_z[i]; logu = ext_logu[i]; logz = ext_logz[i];
        } else {
            const MoveDraw d = draw_move(S, step, half, region, slot - (long long)ridx * halfW);
            ws = d.ws; wc = d.wc; z = d.z; logu = d.logu;
        }
    }
    const RegionDev R = S.regions[region];
    typename PK::Lds& L = lds[PK::SPLIT ? 0 : wave * PK::SUBS + sub];
    VAMP_STAMP(0);
    stretch_move<F32, DRAWS, MODE, PK>(S, R, L, scr[PK::FF ? wave : 0], dct, px, l, wave, red, tabs[PK::SPLIT ? 0 : wave].a, ws, wc, z, logu,
                                       logz, EXT ? -1ll : slot - S.slot_begin);
}

// ---- device-resident step loop (rows a8 / a10 in the regime the reference lives in) -----------------------------------
// The reference's fits are a few thousand iterations of a 4..33-parameter model (vpfits.py:417-428, vpregion.py:42); as
// ensembles of 32..128 walkers per region a launch per half-step is latency-bound (two launches per step, ~10 us each,
// most of it dispatch and the wavefront's own critical path).  Regions are independent posteriors, so ONE workgroup per
// region can run the region's whole step loop: its compute wavefronts take the movers of a half-step in rounds
// (stretch_move: the arithmetic of k_half_step), the half-step barrier is __syncthreads(), the kept samples are written
// from the kernel, and an extra wavefront draws -- one mover per lane, the same Philox keys -- the NEXT half-step's draws
// into an LDS double buffer while the others move.  The chain equals the launch-per-half-step chain bit for bit
// (tests/test_gpu_parity.py::test_resident_step_loop_equals_launch_per_half_step).  No inter-workgroup communication.
constexpr size_t RES_MAX_LDS = 150 * 1024;  // dynamic LDS of one resident workgroup (a workgroup may take all 160 KB of its CU)
constexpr int RES_MAX_REGIONS = 256;        // automatic policy: at most one resident workgroup per compute unit
struct alignas(16) ResDraws {
    double z[RES_MAX_MOVERS], logu[RES_MAX_MOVERS], logz[RES_MAX_MOVERS];
    int ws[RES_MAX_MOVERS], wc[RES_MAX_MOVERS];
};
// layout of the workgroup's dynamic LDS for nw compute wavefronts (host and device compute it alike)
template <bool F32, int MODE, class PK>
struct ResLayout {
    static constexpr size_t up(size_t v) { return (v + 15) & ~(size_t)15; }
    using Tabs = LineTables<table_doubles<F32, MODE, PK>()>;
    static constexpr size_t dct_bytes = PK::FF ? up(ff_table_doubles<F32>() * sizeof(double)) : 0;
    static constexpr size_t off_draws = dct_bytes;
    static constexpr size_t off_red = off_draws + 2 * sizeof(ResDraws);
    __host__ __device__ static constexpr size_t off_scr(int nw) { return off_red + up((size_t)nw * PARTS * sizeof(double)); }
    __host__ __device__ static constexpr size_t off_tabs(int nw) { return off_scr(nw) + (PK::FF ? up((size_t)nw * sizeof(TileScratch)) : 0); }
    __host__ __device__ static constexpr size_t off_lds(int nw) { return off_tabs(nw) + up((size_t)nw * sizeof(Tabs)); }
    __host__ __device__ static constexpr size_t total(int nw) { return off_lds(nw) + up((size_t)nw * PK::SUBS * sizeof(typename PK::Lds)); }
};
template <bool F32, int MODE, class PK>
__global__ __launch_bounds__(64 * (RES_MAX_WAVES + 1), (min_waves<F32, PK>())) void k_run_resident(
    SamplerDev S, PixPtrs px, unsigned step0, long long n_steps, int thin, double* __restrict__ chain, double* __restrict__ lchain,
    long long total_theta, long long total_walkers) {
    static_assert(!PK::SPLIT || PK::WPB == 1, "a walker's group is one wavefront or a part of one");
    using LY = ResLayout<F32, MODE, PK>;
    extern __shared__ __align__(16) unsigned char res_raw[];
    const int nw = (int)(blockDim.x >> 6) - 1;                   // compute wavefronts; wavefront nw draws
    double* dct = reinterpret_cast<double*>(res_raw);
    ResDraws* draws = reinterpret_cast<ResDraws*>(res_raw + LY::off_draws);
    if constexpr (PK::FF) ff_fill_table<F32>(dct);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sub = lane / PK::LPW, l = lane % PK::LPW;
    const bool drawer = wave == nw;
    const int region = __builtin_amdgcn_readfirstlane(S.region_list ? S.region_list[blockIdx.x] : (int)blockIdx.x);
    const RegionDev R = S.regions[region];
    const int halfW = (int)(S.W >> 1);
    const int slots = nw * PK::SUBS;
    const int wv = drawer ? 0 : wave;                             // (the drawing wavefront owns no walker slot)
    double* red = reinterpret_cast<double*>(res_raw + LY::off_red) + wv * PARTS;
    TileScratch& Sx = reinterpret_cast<TileScratch*>(res_raw + LY::off_scr(nw))[PK::FF ? wv : 0];
    double* tab = reinterpret_cast<typename LY::Tabs*>(res_raw + LY::off_tabs(nw))[wv].a;
    typename PK::Lds& L = reinterpret_cast<typename PK::Lds*>(res_raw + LY::off_lds(nw))[wv * PK::SUBS + sub];
    // the draws of one half-step: which walker holds each active slot, its stretch factor, partner and log u
    auto draw_all = [&](unsigned step, int half, ResDraws& D) {
        for (int a = lane; a < halfW; a += 64) {
            const MoveDraw d = draw_move(S, step, half, region, a);
            D.ws[a] = (int)d.ws; D.wc[a] = (int)d.wc; D.z[a] = d.z; D.logu[a] = d.logu; D.logz[a] = log(d.z);
        }
    };
    if (drawer) draw_all(step0, 0, draws[0]);
    __syncthreads();
    long long kept = 0;
    int until_keep = thin;                  // (a countdown: a 64-bit modulo per step is ~100 scalar instructions)
    for (long long it = 0; it < n_steps; ++it) {
        const unsigned step = step0 + (unsigned)it;
        for (int half = 0; half < 2; ++half) {
            const ResDraws& D = draws[half];
            VAMP_STAMP(0);
            if (drawer) {                                          // the next half-step's draws, while the others move
                if (half == 0) draw_all(step, 1, draws[1]);
                else if (it + 1 < n_steps) draw_all(step + 1u, 0, draws[0]);
            } else {
                for (int a0 = 0; a0 < halfW; a0 += slots) {
                    const int a = a0 + wave * PK::SUBS + sub;
                    if (a < halfW)
                        stretch_move<F32, DRAW_PRE, MODE, PK>(S, R, L, Sx, dct, px, l, 0, red, tab, D.ws[a], D.wc[a], D.z[a], D.logu[a],
                                                              D.logz[a], -1ll);
                }
            }
            VAMP_STAMP(7);
            __syncthreads();            // the movers' rows are in place (global, workgroup scope), the next draws are complete
            VAMP_STAMP(8);
        }
        const bool keep_now = --until_keep == 0;
        if (keep_now) until_keep = thin;
        if (keep_now && (chain || lchain)) {
            if (chain) {
                const double* __restrict__ src = S.X + R.theta_off;
                double* __restrict__ dst = chain + kept * total_theta + R.theta_off;
                for (long long e = tid; e < S.W * R.D; e += blockDim.x) dst[e] = src[e];
            }
            if (lchain) {
                const double* __restrict__ src = S.lnp + R.walker_off;
                double* __restrict__ dst = lchain + kept * total_walkers + R.walker_off;
                for (long long e = tid; e < S.W; e += blockDim.x) dst[e] = src[e];
            }
            ++kept;
            __syncthreads();            // (the next half-step moves rows this copy reads)
        }
    }
}

// Walker-sharded runs: rows of the active colour gathered from every device, in slot order
// (recv[i] = slot first_slot + i, D + 1 doubles: position and lnprob), are written to the walkers
// that hold those slots in this (step, half).  16 lanes per row; rows [own_lo, own_hi) are this
// device's own movers, already in place.
__global__ __launch_bounds__(256) void k_scatter_rows(SamplerDev S, const double* __restrict__ recv, unsigned step, int half,
                                                      long long first_slot, long long n_rows, long long own_lo, long long own_hi) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (i >= n_rows || (i >= own_lo && i < own_hi)) return;
    const RegionDev& R = S.regions[0];
    const int D = R.D;
    const long long slot = first_slot + i;
    const unsigned hb = (unsigned)(S.split_block >> 1);
    const unsigned chunk = (unsigned)(slot / hb), pos = (unsigned)(slot % hb);
    const long long ws = (long long)chunk * S.split_block +
                         vamp::split_perm(S.seed, step, chunk, (unsigned)R.rng_id, pos + (half ? hb : 0u), (unsigned)S.split_block);
    const double* src = recv + i * (long long)(D + 1);
    double* dst = S.X + R.theta_off + ws * D;
    for (int d = l; d < D; d += 16) dst[d] = src[d];
    if (l == 0) S.lnp[R.walker_off + ws] = src[D];
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
using vamp::fail;
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (void)hipGetLastError();   /* reported here: do not leave it for the next library (RCCL) to find */ \
            return fail(e_ == hipErrorOutOfMemory ? VAMP_ERR_NOMEM : VAMP_ERR_HIP,            \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                   \
        }                                                                                     \
    } while (0)

// n elements of T in device memory (PINNED: page-locked host memory the kernels read and write directly), owned:
// released by reset() and on destruction.  ensure(n) grows it to at least n elements, contents not kept; the capacity
// is recorded only once the allocation has succeeded.
template <class T, bool PINNED = false>
class Buf {
  public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    ~Buf() { reset(); }
    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    hipError_t ensure(size_t n) {
        if (cap_ >= n) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }
  private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <class T> using DevBuf = Buf<T>;
template <class T> using PinnedBuf = Buf<T, true>;

// run the statement with `M` bound to the compile-time parameterisation that matches runtime
// `mode`, `PK` to the Pack type of launch shape `shape` and `F32` to the context's precision
#define VAMP_FOR_MODE_(mode, ...)                                               \
    do {                                                                        \
        if ((mode) == VAMP_GAUSS3) { constexpr int M = VAMP_GAUSS3; __VA_ARGS__; } \
        else if ((mode) == VAMP_VOIGT4) { constexpr int M = VAMP_VOIGT4; __VA_ARGS__; } \
        else { constexpr int M = VAMP_NBZ3; __VA_ARGS__; }                      \
    } while (0)
#define VAMP_FOR_MODE(mode, ...) VAMP_FOR_MODE_(mode, __VA_ARGS__)
#define VAMP_FOR_F32(f32, ...)                                                  \
    do {                                                                        \
        if (f32) { constexpr bool F32 = true; __VA_ARGS__; }                    \
        else { constexpr bool F32 = false; __VA_ARGS__; }                       \
    } while (0)
// launch shapes (see struct Pack): what one launch class of a context runs
enum Shape { SH_SMALL = 0, SH_MID = 1, SH_WIDE = 2, SH_WIDE_FULL = 3, SH_SPLIT = 4, SH_SPLIT_FULL = 5, SH_SMALL2 = 6, SH_XL = 7 };
#define VAMP_FOR_PK(shape, ...)                                                 \
    do {                                                                        \
        if ((shape) == SH_SMALL) { using PK = PackSmall; __VA_ARGS__; }         \
        else if ((shape) == SH_SMALL2) { using PK = PackSmall2; __VA_ARGS__; }  \
        else if ((shape) == SH_MID) { using PK = PackMid; __VA_ARGS__; }        \
        else if ((shape) == SH_XL) { using PK = PackXL; __VA_ARGS__; }          \
        else if ((shape) == SH_SPLIT_FULL) { using PK = PackSplitFull; __VA_ARGS__; } \
        else if ((shape) == SH_SPLIT) { using PK = PackSplit; __VA_ARGS__; }    \
        else if ((shape) == SH_WIDE_FULL) { using PK = PackWideFull; __VA_ARGS__; } \
        else { using PK = PackWide; __VA_ARGS__; }                              \
    } while (0)
#define VAMP_FOR_MODE_PK(f32, mode, shape, ...) VAMP_FOR_F32(f32, VAMP_FOR_PK(shape, VAMP_FOR_MODE_(mode, __VA_ARGS__)))
inline long long shape_walkers_per_block(int sh) { long long v = 0; VAMP_FOR_PK(sh, v = PK::WALKERS_PER_BLOCK); return v; }
inline long long shape_waves(int sh) { long long v = 0; VAMP_FOR_PK(sh, v = PK::WPB); return v; }
inline unsigned shape_threads(int sh) { unsigned v = 0; VAMP_FOR_PK(sh, v = PK::THREADS); return v; }

// A launch class: the regions of a context that one kernel shape serves.  Real spectra mix many
// short single-line regions (four walkers per wavefront) with a few long blends (a wavefront per
// walker with Taylor tables); each class is one launch per half-step over its own region list.
using vamp::plan::CK_SMALL; using vamp::plan::CK_MID; using vamp::plan::CK_WIDE; using vamp::plan::CK_SMALL2; using vamp::plan::CK_XL;
struct LaunchClass {
    int kind = CK_WIDE;
    std::vector<int> regions;
    DevBuf<int> list_d;          // device copy of `regions`; empty when the class is every region in order
};

// HIP event pairs around intervals of a stream's work (a half-step's launches, an exchange): begin() records an
// interval's opening event, end() its closing one, flush() adds the closed intervals to ms and n.  At most 4096 pairs
// are kept: begin() flushes a full set before it reuses them.
struct EventPairs {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;             // closed intervals not yet flushed; ev[used] is the one begin() opened
    double ms = 0.0;
    long long n = 0;
    EventPairs() = default;
    EventPairs(const EventPairs&) = delete;
    EventPairs& operator=(const EventPairs&) = delete;
    ~EventPairs() {
        for (auto& p : ev) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    }
    int begin(hipStream_t st) {
        if (used == ev.size()) {
            if (ev.size() >= 4096) {
                int rc = flush();
                if (rc) return rc;
            } else {
                hipEvent_t a, b;
                HIP_TRY(hipEventCreate(&a));
                HIP_TRY(hipEventCreate(&b));
                ev.emplace_back(a, b);
            }
        }
        HIP_TRY(hipEventRecord(ev[used].first, st));
        return 0;
    }
    int end(hipStream_t st) {
        HIP_TRY(hipEventRecord(ev[used].second, st));
        ++used;
        return 0;
    }
    int flush() {
        for (size_t i = 0; i < used; ++i) {
            float t = 0.f;
            HIP_TRY(hipEventSynchronize(ev[i].second));
            HIP_TRY(hipEventElapsedTime(&t, ev[i].first, ev[i].second));
            ms += t;
            n += 1;
        }
        used = 0;
        return 0;
    }
};

}  // namespace

// the state the host implementation of the ABI shares (vamp::AbiState: regions, class plan, sampler scalars, shard and
// part bookkeeping, communicator) and what lives on the device
struct vamp_ctx : vamp::AbiState {
    int device = 0;
    int wofz_kind = VAMP_WOFZ_ACCURATE;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // the launch classes of plan and plan_small (vamp_set_regions): one launch per class and half-step
    std::vector<LaunchClass> classes;
    std::vector<LaunchClass> classes_small;
    // draws of packed launches (k_draws), grown on demand
    DevBuf<int> dr_ws, dr_wc;
    DevBuf<double> dr_z, dr_lu, dr_lz;
    // launch classes of one half-step run concurrently, each on its own stream (forked from and joined
    // to the ctx stream with events): a class of low-occupancy blends and a class of register-bound
    // short regions fill each other's stalls
    bool concurrent_classes = true;
    std::vector<hipStream_t> cls_stream;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_join;
    DevBuf<RegionDev> regions_d;
    long long n_pix = 0;
    DevBuf<double> x_d, f_d, wt_d;
    DevBuf<float> xf_d, ff_d, wtf_d;
    // the state: X_d / lnp_d are the walkers' positions and lnprobs, in X_own / lnp_own or in the caller's memory
    // (vamp_sampler_bind_state)
    double* X_d = nullptr;
    double* lnp_d = nullptr;
    DevBuf<double> X_own, lnp_own;
    DevBuf<long long> nacc_d;
    // walker-sharded runs: the exchange buffers (AbiState::exchange), see vamp_comm_*
    DevBuf<double> send_d;           // [parts][part_slots][D + 1]
    DevBuf<double> recv_d;           // [parts][world * part_slots][D + 1]
    void* rccl = nullptr;            // ncclComm_t (RCCL), one per ctx
    hipStream_t comm_stream = nullptr;
    std::vector<hipEvent_t> ev_kernel, ev_scatter;   // per part: kernel done / rows scattered
    // exchange timing (vamp_exchange_timing): event pairs around all-gather + scatter on the stream they run on
    EventPairs xtiming;
    // grow-only scratch of vamp_lnprob (the MAP optimiser calls it thousands of times with W = 1)
    DevBuf<double> sc_th, sc_lp, sc_chi;
    // small evaluations (the MAP searches: a few points per region, thousands of times): pinned host memory the
    // kernel reads and writes directly -- no staging copies, one launch and one synchronisation per call
    PinnedBuf<double> pin_th, pin_out;
    // the MAP searches on the device (k_map_search): start points, flags, simplices, results; grow-only
    DevBuf<double> map_th_d, map_best_d, map_sim_d;
    DevBuf<unsigned char> map_act_d;
    DevBuf<long long> map_it_d;
    // run-time options (vamp_ctx_set_option)
    int opt_map_device = 1;          // 1: vamp_map_all runs k_map_search; 0: the host-driven search, one launch per iteration
    int opt_resident = 1;            // 1: small ensembles are stepped by the device-resident loop where it pays (resident_eligible);
                                     // 0: never; 2: wherever the kernel can run
    // scratch for the ext hook
    DevBuf<int> ext_act_d, ext_par_d;
    DevBuf<double> ext_z_d, ext_lu_d;
    // kernel timing: one interval per launch_half / run_resident call
    bool timing = false;
    EventPairs ktiming;

    // far-field tables of the regions' full tiles (k_tile_tables, launched by vamp_set_regions): one real per pixel and
    // two doubles per 256 pixels; empty when no region has a full tile the far-field sweep could run on
    DevBuf<double> u_d;
    DevBuf<float> uf_d;
    DevBuf<double2> geo_d;
    DevBuf<double> mom_d;            // (fp64 contexts built with VAMP_TILE_MOMENTS: MOM_TILE doubles per slot of geo_d)

    PixPtrs pix() const {
        return PixPtrs{x_d.get(), f_d.get(), wt_d.get(), xf_d.get(), ff_d.get(), wtf_d.get(), u_d.get(), uf_d.get(), geo_d.get(), mom_d.get()};
    }
};

namespace {

// forgets the regions and their launch classes
void reset_regions(vamp_ctx* c) {
    c->regions_d.reset();
    c->x_d.reset(); c->f_d.reset(); c->wt_d.reset();
    c->xf_d.reset(); c->ff_d.reset(); c->wtf_d.reset();
    c->u_d.reset(); c->uf_d.reset(); c->geo_d.reset(); c->mom_d.reset();
    c->classes.clear();
    c->classes_small.clear();
    c->n_regions = 0;
}

// forgets the state, also a bound one (vamp_sampler_bind_state)
void reset_sampler(vamp_ctx* c) {
    c->X_own.reset(); c->lnp_own.reset();
    c->X_d = c->lnp_d = nullptr;
    c->nacc_d.reset();
    c->send_d.reset(); c->recv_d.reset();
    c->exchange = false;
    c->sampler_ready = false;
}

// exchange buffers of the shard set by vamp_sampler_set_shard_parts: the movers of every part in slot order,
// position + lnprob per row (+ the per-part events when a communicator will run the exchange)
int ensure_part_events(vamp_ctx* c, int parts);
int alloc_exchange_buffers(vamp_ctx* c) {
    HIP_TRY(c->send_d.ensure(vamp::exchange_send_doubles(c)));
    HIP_TRY(c->recv_d.ensure(vamp::exchange_recv_doubles(c)));
    vamp::exchange_parts(c);
    c->exchange = true;
    if (c->comm) return ensure_part_events(c, c->shard_parts);
    return 0;
}

// per-part events of the overlapped exchange (kernel of a part done / its rows scattered)
int ensure_part_events(vamp_ctx* c, int parts) {
    while ((int)c->ev_kernel.size() < parts) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        c->ev_kernel.push_back(a);
        c->ev_scatter.push_back(b);
    }
    return 0;
}

// kernel shape of launch class `cl` for an ensemble with `per_region` movers per region and half-step and `total` movers
// per launch of the class -- UNSHARDED counts (W/2 of a walker-sharded single-region ensemble, whatever this device's share
// or piece of it), so that a shard runs the shape, the same bits, the whole ensemble runs on one device.
// The packed shapes (several walkers per wavefront: the fixed work of a wavefront shared) are the throughput shapes: launches
// that fill the chip (>= PACK_MIN_WALKERS movers), and the small ensembles of model-selection ladders (<= RES_MAX_MOVERS
// movers per region: tens of regions x tens of walkers, where they also feed the device-resident loop -- and single points:
// vamp_lnprob, the MAP search).  In between -- config 2: one region, 4096 walkers -- a launch cannot fill the chip and is
// bound by one wavefront's critical path: one walker per wavefront (14 us per half-step against 23 packed,
// profiles/r04_c_small_ensembles.txt).  All callers of one context ask with the same counts.
// the launch classes an ensemble of `per_region` movers per region and half-step runs in (callers of one context ask with
// the same count: the sampler and the resident loop with W / 2, vamp_lnprob(_all) of W points with W / 2, the MAP search with 1)
inline bool small_ensemble(long long per_region) { return per_region <= RES_MAX_MOVERS; }
const std::vector<LaunchClass>& partition_for(const vamp_ctx* c, long long per_region) {
    return small_ensemble(per_region) ? c->classes_small : c->classes;
}
const std::vector<int>& class_of_for(const vamp_ctx* c, long long per_region) {
    return small_ensemble(per_region) ? c->plan_small.class_of : c->plan.class_of;
}
int class_shape(const vamp_ctx* c, const LaunchClass& cl, long long per_region, long long total, bool packable) {
    if (cl.kind == CK_XL) return SH_XL;
    if (cl.kind == CK_MID) return SH_MID;
    if ((cl.kind == CK_SMALL || cl.kind == CK_SMALL2) && packable &&
        (c->packing == 16 || per_region <= RES_MAX_MOVERS || total >= PACK_MIN_WALKERS)) {
        // one- and two-line regions: eight lanes per walker is the throughput shape (six pixels per lane of a 44-pixel
        // region: 14 800 clocks of sweep per half-step, in-kernel stamps); a small ensemble is bound by exactly that critical
        // path and runs sixteen lanes per walker (three pixels per lane: 8 300; profiles/r04_c_small_ensembles.txt) -- as
        // part of the merged short-region class
        // (small ensembles never see CK_SMALL2: their partition has the short-region classes merged, partition_for)
        return cl.kind == CK_SMALL2 ? SH_SMALL2 : SH_SMALL;
    }
    const bool split = cl.kind == CK_WIDE && (c->packing == 256 || (c->packing == 0 && c->plan.min_tiles >= 2 * PARTS));
    if (split) return c->plan.full_tiles ? SH_SPLIT_FULL : SH_SPLIT;
    return c->plan.full_tiles ? SH_WIDE_FULL : SH_WIDE;
}
// movers of one launch of class `cl` when every region holds `per_region` movers (what decides the class's shape): a
// single-region ensemble is one launch of its movers -- a shard or a piece of it takes the shape of the whole
long long class_movers(const vamp_ctx* c, const LaunchClass& cl, long long per_region) {
    return c->n_regions == 1 ? per_region : (long long)cl.regions.size() * per_region;
}
// the shape class `cl` runs in for `per_region` movers per region: the one rule behind the sampler's launches
// (launch_half, run_resident), vamp_lnprob(_all) and the MAP search (and the test hook vampdbg_launch_plan)
int launch_shape(const vamp_ctx* c, const LaunchClass& cl, long long per_region) {
    return class_shape(c, cl, per_region, class_movers(c, cl, per_region), true);
}
// movers per region the entry points ask with.  W points per region are W/2 movers of a W-walker ensemble: the sampler's
// own initial log-posteriors, and a caller's walker checks, run the classes and shapes the ensemble will be stepped in
inline long long lnprob_movers(long long W) { return (W + 1) / 2; }
constexpr long long MAP_MOVERS = 1;      // the MAP search: the shape vamp_lnprob runs a single point in

// the SamplerDev fields every sampler launch shares, the others zero
SamplerDev sampler_dev(const vamp_ctx* c) {
    SamplerDev S;
    std::memset(&S, 0, sizeof(S));
    S.regions = c->regions_d.get();
    S.n_regions = c->n_regions;
    S.W = c->W;
    S.split_block = c->split_block;
    S.a = c->a;
    S.seed = c->seed;
    S.X = c->X_d;
    S.lnp = c->lnp_d;
    S.n_accept = c->nacc_d.get();
    return S;
}

// the launch classes of a half-step (launch_half, run_resident) on forked streams: class 0 runs on the ctx stream,
// class ci > 0 on cls_stream[ci - 1], which starts at the fork point recorded here on the ctx stream ...
int fork_classes(vamp_ctx* c, size_t ncls) {
    while (c->cls_stream.size() < ncls - 1) {
        hipStream_t st;
        hipEvent_t ev;
        HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->cls_stream.push_back(st);
        c->ev_join.push_back(ev);
    }
    if (!c->ev_fork) HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
    for (size_t ci = 1; ci < ncls; ++ci) HIP_TRY(hipStreamWaitEvent(c->cls_stream[ci - 1], c->ev_fork, 0));
    return 0;
}
// ... and which the ctx stream waits for again once class ci is launched
int join_class(vamp_ctx* c, size_t ci) {
    if (ci == 0) return 0;
    HIP_TRY(hipEventRecord(c->ev_join[ci - 1], c->cls_stream[ci - 1]));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join[ci - 1], 0));
    return 0;
}

// One half-step of this ctx's share (piece `part` of it): one launch per launch class, on the ctx
// stream.  ext: host-supplied draws for `ext_n` movers of `ext_region`.
int launch_half(vamp_ctx* c, int half, bool ext, int ext_region, long long ext_n, int part = 0) {
    SamplerDev S = sampler_dev(c);
    if (!ext && c->exchange) {
        S.pack = c->send_d.get() + (long long)part * c->part_slots * (c->regions_h[0].D + 1);
        c->part_step[part] = (unsigned)c->step;
        c->part_half[part] = half;
    }
    int rc = c->timing ? c->ktiming.begin(c->stream) : 0;
    if (rc) return rc;
    const unsigned step = (unsigned)c->step;
    const PixPtrs px = c->pix();
    const long long halfW = c->W / 2;
    const int* ni = nullptr;
    const double* nd = nullptr;
    // several walkers per wavefront need every wavefront inside one region: trivially so with one region, else the
    // wavefronts are dealt per region (SamplerDev::wpr); host-supplied draws run one walker per wavefront
    const bool packable = !ext;
    const std::vector<LaunchClass>& classes = partition_for(c, halfW);
    const std::vector<int>& class_of = class_of_for(c, halfW);
    const size_t ncls = classes.size();
    // the classes of a half-step on forked streams fill each other's stalls when the launches are big (config 3: 4.85 ->
    // 4.20 ms); for the small ensembles of a ladder the event traffic of fork and join costs more than it hides
    // (q1422 ladder, first rung: 73 -> 57 us per half-step without it)
    const bool fork = !ext && ncls > 1 && c->concurrent_classes && c->total_walkers / 2 >= PACK_MIN_WALKERS * 4;
    rc = fork ? fork_classes(c, ncls) : 0;
    if (rc) return rc;
    // draws of the packed classes: one slice of the buffers per class (the classes may overlap in time)
    long long draw_total = 0;
    if (!ext)
        for (const LaunchClass& cl : classes) draw_total += (c->n_regions == 1) ? c->total_walkers : (long long)cl.regions.size() * halfW;
    long long draw_off = 0;
    for (size_t ci = 0; ci < ncls; ++ci) {
        const LaunchClass& cl = classes[ci];
        if (ext && class_of[ext_region] != (int)ci) continue;
        long long n;
        if (ext) {
            n = ext_n;
        } else if (c->n_regions == 1) {          // possibly a shard / a piece of one
            S.slot_begin = c->slot_begin + part * c->part_stride;
            S.slot_end = c->shard_parts > 1 ? S.slot_begin + c->part_slots : c->slot_end;
            n = S.slot_end - S.slot_begin;
        } else {
            S.slot_begin = 0;
            S.slot_end = (long long)cl.regions.size() * halfW;
            n = S.slot_end;
        }
        if (n <= 0) continue;
        const hipStream_t st = (fork && ci > 0) ? c->cls_stream[ci - 1] : c->stream;
        S.region_list = cl.list_d.get();
        // (a shard or a piece of a single-region ensemble takes the shape of the WHOLE ensemble)
        const int shape = ext ? class_shape(c, cl, n, n, packable) : launch_shape(c, cl, halfW);
        unsigned grid = (unsigned)((n + shape_walkers_per_block(shape) - 1) / shape_walkers_per_block(shape));
        S.wpr = S.bpr = 0;
        S.n_cls_regions = (int)cl.regions.size();
        if (!ext && c->n_regions > 1 && (shape == SH_SMALL || shape == SH_SMALL2)) {
            const vamp::plan::PackedGrid pg = vamp::plan::plan_packed_grid((long long)cl.regions.size(), halfW,
                                                                           shape == SH_SMALL ? PackSmall::SUBS : PackSmall2::SUBS,
                                                                           shape == SH_SMALL ? PackSmall::WPB : PackSmall2::WPB);
            S.wpr = pg.wpr;
            S.bpr = pg.bpr;
            grid = (unsigned)pg.grid;
        } else if (!ext && c->n_regions > 1 && halfW % shape_walkers_per_block(shape) == 0) {
            S.bpr = (int)(halfW / shape_walkers_per_block(shape));        // one walker per wavefront or per workgroup
        }
        const dim3 threads(shape_threads(shape));
        if (ext) {
            VAMP_FOR_MODE_PK(c->f32, c->mode, shape, hipLaunchKernelGGL((k_half_step<F32, DRAW_HOST, M, PK>), dim3(grid), threads, 0, st, S, px, step,
                                                                    half, ext_region, ext_n, c->ext_act_d.get(), c->ext_par_d.get(),
                                                                    c->ext_z_d.get(), c->ext_lu_d.get(), nd));
        } else if (!small_ensemble(halfW) && (shape == SH_SMALL || shape == SH_SMALL2 || (shape == SH_MID && VAMP_MID_PREDRAW))) {
            // four walkers per wavefront (or a walker per wavefront at ~1.7 wavefronts per SIMD, where
            // ~1000 scalar instructions of draws are exposed latency): draws in their own
            // one-thread-per-mover launch -- for ensembles that fill the chip; a small ensemble's half-step is bound by
            // its launches, and draws in the kernel are one launch less (the same draws: same keys, same functions)
            HIP_TRY(c->dr_ws.ensure(draw_total));
            HIP_TRY(c->dr_wc.ensure(draw_total));
            HIP_TRY(c->dr_z.ensure(draw_total));
            HIP_TRY(c->dr_lu.ensure(draw_total));
            HIP_TRY(c->dr_lz.ensure(draw_total));
            int *d_ws = c->dr_ws.get() + draw_off, *d_wc = c->dr_wc.get() + draw_off;
            double *d_z = c->dr_z.get() + draw_off, *d_lu = c->dr_lu.get() + draw_off, *d_lz = c->dr_lz.get() + draw_off;
            draw_off += n;
            hipLaunchKernelGGL(k_draws, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, step, half, n, d_ws, d_wc, d_z, d_lu, d_lz);
            HIP_TRY(hipGetLastError());
            VAMP_FOR_MODE_PK(c->f32, c->mode, shape, hipLaunchKernelGGL((k_half_step<F32, DRAW_PRE, M, PK>), dim3(grid), threads, 0, st, S, px, step,
                                                                    half, 0, 0ll, d_ws, d_wc, d_z, d_lu, d_lz));
        } else {
            VAMP_FOR_MODE_PK(c->f32, c->mode, shape, hipLaunchKernelGGL((k_half_step<F32, DRAW_INLINE, M, PK>), dim3(grid), threads, 0, st, S, px, step,
                                                                    half, 0, 0ll, ni, ni, nd, nd, nd));
        }
        HIP_TRY(hipGetLastError());
        rc = fork ? join_class(c, ci) : 0;
        if (rc) return rc;
    }
    return c->timing ? c->ktiming.end(c->stream) : 0;
}

// ---- the device-resident step loop (k_run_resident): eligibility and launch ----------------------------------------
// compute wavefronts of a resident workgroup of shape PK for `movers` movers per half-step, or 0: does not fit
template <bool F32, int MODE, class PK>
int resident_waves(long long movers) {
    if constexpr (PK::SPLIT && PK::WPB > 1) return 0;
    else {
        int nw = (int)std::min<long long>(RES_MAX_WAVES, (movers + PK::SUBS - 1) / PK::SUBS);
        while (nw > 0 && ResLayout<F32, MODE, PK>::total(nw) > RES_MAX_LDS) --nw;
        return nw;
    }
}
template <bool F32, int MODE, class PK>
int launch_resident(int device, dim3 grid, dim3 threads, int nw, hipStream_t st, const SamplerDev& S, const PixPtrs& px, unsigned step0,
                    long long n_steps, int thin, double* chain_dev, double* lchain_dev, long long total_theta, long long total_walkers) {
    if constexpr (!(PK::SPLIT && PK::WPB > 1)) {    // (resident_waves is 0 for the workgroup-per-walker shapes: never launched)
        using LY = ResLayout<F32, MODE, PK>;
        const size_t lds = LY::total(nw);
        // beyond the default dynamic allocation the kernel must be told, once per device (bit d of `told`: device d)
        static std::atomic<unsigned long long> told{0};
        const unsigned long long bit = device < 64 ? 1ull << device : 0ull;
        if (lds > 48 * 1024 && !(told.load() & bit)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_run_resident<F32, MODE, PK>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)RES_MAX_LDS);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(VAMP_ERR_HIP, "hipFuncSetAttribute(k_run_resident<F32=" + std::to_string(F32) + ", MODE=" + std::to_string(MODE) +
                                              ", LPW=" + std::to_string(PK::LPW) + ", WPB=" + std::to_string(PK::WPB) + ">, " +
                                              "MaxDynamicSharedMemorySize, " + std::to_string(RES_MAX_LDS) + " bytes): " + hipGetErrorString(e));
            }
            told.fetch_or(bit);
        }
        hipLaunchKernelGGL((k_run_resident<F32, MODE, PK>), grid, threads, lds, st, S, px, step0, n_steps, thin, chain_dev, lchain_dev,
                           total_theta, total_walkers);
    }
    return 0;
}
int resident_waves_for(const vamp_ctx* c, int shape, long long movers) {
    int nw = 0;
    VAMP_FOR_MODE_PK(c->f32, c->mode, shape, nw = resident_waves<F32, M, PK>(movers));
    return nw;
}
// dynamic LDS bytes of a resident workgroup of shape PK with nw compute wavefronts (what launch_resident asks for)
template <bool F32, int MODE, class PK>
long long resident_lds(int nw) {
    if constexpr (PK::SPLIT && PK::WPB > 1) return 0;
    else return (long long)ResLayout<F32, MODE, PK>::total(nw);
}
// every launch class of the context can run its regions' step loops inside one launch each
// Policy (opt_resident = 1; measured, profiles/r04_c_small_ensembles.txt).  A resident workgroup removes the dispatch
// gap of a launch per half-step (~5 us of ~16) but serialises its region on ONE compute unit, so it pays only where
// the launch path cannot use the chip anyway: at most one workgroup per compute unit (<= RES_MAX_REGIONS regions),
// every mover of a half-step in ONE round of the workgroup's wavefronts, and only the packed short-region classes
// (a blend or a region of 17+ lines takes a whole wavefront per walker: eight movers per round).  opt_resident = 2
// (tests, A/B) takes every context the kernel can run.
bool resident_eligible(const vamp_ctx* c) {
    if (!c->opt_resident || !c->sampler_ready) return false;
    if (c->shard_world != 1 || c->shard_parts != 1 || c->comm || c->exchange) return false;     // walker-sharded: the exchange is per half-step
    const long long halfW = c->W / 2;
    if (halfW > RES_MAX_MOVERS) return false;
    if (c->opt_resident == 1 && c->n_regions > RES_MAX_REGIONS) return false;
    for (const LaunchClass& cl : partition_for(c, halfW)) {
        const int shape = launch_shape(c, cl, halfW);
        const int nw = resident_waves_for(c, shape, halfW);
        if (!vamp::plan::resident_class_ok(cl.kind, halfW, nw, (int)(shape_walkers_per_block(shape) / shape_waves(shape)), c->opt_resident == 1))
            return false;
    }
    return true;
}
// n_steps of every region, one launch per launch class (the classes on forked streams, as in launch_half)
int run_resident(vamp_ctx* c, long long n_steps, int thin, double* chain_dev, double* lchain_dev) {
    SamplerDev S = sampler_dev(c);
    const long long halfW = c->W / 2;
    const std::vector<LaunchClass>& classes = partition_for(c, halfW);
    const size_t ncls = classes.size();
    const bool fork = ncls > 1 && c->concurrent_classes;
    int rc = c->timing ? c->ktiming.begin(c->stream) : 0;
    if (rc) return rc;
    rc = fork ? fork_classes(c, ncls) : 0;
    if (rc) return rc;
    const PixPtrs px = c->pix();
    for (size_t ci = 0; ci < ncls; ++ci) {
        const LaunchClass& cl = classes[ci];
        const hipStream_t st = (fork && ci > 0) ? c->cls_stream[ci - 1] : c->stream;
        S.region_list = cl.list_d.get();
        const int shape = launch_shape(c, cl, halfW);     // the shape launch_half runs this class in
        const int nw = resident_waves_for(c, shape, halfW);
        const dim3 grid((unsigned)cl.regions.size()), threads(64u * (unsigned)(nw + 1));
        VAMP_FOR_MODE_PK(c->f32, c->mode, shape, rc = launch_resident<F32, M, PK>(c->device, grid, threads, nw, st, S, px, (unsigned)c->step,
                                                                                 n_steps, thin, chain_dev, lchain_dev, c->total_theta,
                                                                                 c->total_walkers));
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        rc = fork ? join_class(c, ci) : 0;
        if (rc) return rc;
    }
    rc = c->timing ? c->ktiming.end(c->stream) : 0;
    if (rc) return rc;
    c->step += n_steps;
    return 0;
}

// ---- RCCL, bound at run time ------------------------------------------------------------------
// Only walker-sharded multi-GPU runs need it, so the library does not link librccl: the few entry
// points are resolved with dlopen on first use (the copy already mapped into the process, e.g. by
// torch, wins; else /opt/rocm/lib).  Prototypes as in rccl/rccl.h (NCCL API).
struct RcclUniqueId { char internal[VAMP_COMM_ID_BYTES]; };
struct RcclApi {
    int (*GetUniqueId)(RcclUniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, RcclUniqueId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;        // optional: vamp_comm_info asks the communicator itself
    int (*CommUserRank)(void*, int*) = nullptr;
    bool ok = false;
};
constexpr int RCCL_FLOAT64 = 8;       // ncclFloat64 / ncclDouble

int rccl_api(RcclApi** out) {
    static RcclApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        void* h = nullptr;
        // VAMP_RCCL_LIB: a library with the five NCCL entry points used here, tried first.  The GPU tests
        // point it at a stand-in that moves the bytes through host shared memory (tests/host/rccl_fake.cpp),
        // which lets two ranks share the one GPU of a test box -- RCCL itself refuses that -- and runs the
        // whole in-library exchange path at world > 1.
        if (const char* over = getenv("VAMP_RCCL_LIB")) h = dlopen(over, RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            // RCCL must sit on the SAME HIP / HSA runtime as this library: a process that also imports torch holds
            // torch's private copies (torch/lib/libamdhip64.so, libhsa-runtime64.so, librccl.so) beside the system
            // ones, and an RCCL bound to a runtime nobody initialised fails in ncclCommInitRank ("no ROCm-capable
            // device is detected") -- which copy a bare dlopen("librccl.so") returns depends on the import order.
            // So: first the librccl next to the libamdhip64 this library is linked against, then the usual names.
            std::vector<std::string> names;
            Dl_info info;
            if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &info) && info.dli_fname) {
                std::string dir(info.dli_fname);
                const size_t cut = dir.rfind('/');
                if (cut != std::string::npos) {
                    dir.resize(cut);
                    names.push_back(dir + "/librccl.so.1");
                    names.push_back(dir + "/librccl.so");
                }
            }
            for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) names.push_back(n);
            for (const std::string& name : names) {
                h = dlopen(name.c_str(), RTLD_NOW | RTLD_GLOBAL);
                if (h) break;
            }
        }
        if (h) {
            api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
            api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
            api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
            api.AllGather = (decltype(api.AllGather))dlsym(h, "ncclAllGather");
            api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
            api.CommCount = (decltype(api.CommCount))dlsym(h, "ncclCommCount");
            api.CommUserRank = (decltype(api.CommUserRank))dlsym(h, "ncclCommUserRank");
            api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather && api.GetErrorString;
        }
    }
    if (!api.ok) return fail(VAMP_ERR_COMM, "RCCL is not available (librccl.so could not be loaded)");
    *out = &api;
    return VAMP_OK;
}
#define RCCL_TRY(api, expr)                                                                   \
    do {                                                                                      \
        int r_ = (expr);                                                                      \
        if (r_ != 0) return fail(VAMP_ERR_COMM, std::string(#expr) + ": " + (api)->GetErrorString(r_)); \
    } while (0)

// ---- roctx ranges (SURVEY section 5 "Tracing"), bound at run time like RCCL ----------------------
// `rocprofv3 --marker-trace` shows the sampler loop, every half-step (with its exchange), the MAP searches and
// the batched evaluations as named ranges around the kernels.  Without a tool attached a range costs two calls
// into an idle library; VAMP_ROCTX=0 switches them off altogether.
struct RoctxApi {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
RoctxApi* roctx_api() {
    static RoctxApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        const char* sw = getenv("VAMP_ROCTX");
        if (sw && std::atoi(sw) == 0) return nullptr;
        std::vector<std::string> names;
        Dl_info info;
        if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t cut = dir.rfind('/');
            if (cut != std::string::npos) {
                dir.resize(cut);
                names.push_back(dir + "/librocprofiler-sdk-roctx.so.1");
                names.push_back(dir + "/libroctx64.so.4");
            }
        }
        for (const char* n : {"librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1",
                              "/opt/rocm/lib/libroctx64.so.4"})
            names.push_back(n);
        for (const std::string& name : names) {
            void* h = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (!h) continue;
            api.push = (decltype(api.push))dlsym(h, "roctxRangePushA");
            api.pop = (decltype(api.pop))dlsym(h, "roctxRangePop");
            if (api.push && api.pop) break;
            api.push = nullptr;
            api.pop = nullptr;
        }
    }
    return (api.push && api.pop) ? &api : nullptr;
}
struct RoctxRange {
    RoctxApi* a;
    explicit RoctxRange(const char* name) : a(roctx_api()) { if (a) a->push(name); }
    ~RoctxRange() { if (a) a->pop(); }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};

// rows of part `part` gathered in c->recv_d -> walker rows (on `st`)
int launch_scatter(vamp_ctx* c, int part, hipStream_t st) {
    const SamplerDev S = sampler_dev(c);
    const long long n_rows = (long long)c->shard_world * c->part_slots;
    const long long own_lo = (long long)c->shard_rank * c->part_slots;
    const double* recv = c->recv_d.get() + part * vamp::part_doubles(c, true);
    const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
    hipLaunchKernelGGL(k_scatter_rows, dim3(grid), dim3(256), 0, st, S, recv, c->part_step[part], c->part_half[part],
                       (long long)part * c->part_stride, n_rows, own_lo, own_lo + c->part_slots);
    HIP_TRY(hipGetLastError());
    return 0;
}

// after launch_half(part): all-gather the part's movers over RCCL and scatter them.  With several
// parts the exchange runs on the communication stream, so that it overlaps the next part's kernel.
int exchange_part(vamp_ctx* c, int part) {
    RcclApi* api = nullptr;
    int rc = rccl_api(&api);
    if (rc) return rc;
    const size_t count = vamp::part_doubles(c, false);
    const double* send = c->send_d.get() + part * count;
    double* recv = c->recv_d.get() + part * vamp::part_doubles(c, true);
    const bool overlap = c->shard_parts > 1;
    hipStream_t st = overlap ? c->comm_stream : c->stream;
    if (overlap) {
        rc = ensure_part_events(c, c->shard_parts);     // (whichever of set_shard_parts / comm_init_rank came first)
        if (rc) return rc;
        HIP_TRY(hipEventRecord(c->ev_kernel[part], c->stream));
        HIP_TRY(hipStreamWaitEvent(c->comm_stream, c->ev_kernel[part], 0));
    }
    rc = c->timing ? c->xtiming.begin(st) : 0;
    if (rc) return rc;
    const int r_ = api->AllGather(send, recv, count, RCCL_FLOAT64, c->rccl, st);
    if (r_ != 0) return fail(VAMP_ERR_COMM, std::string("ncclAllGather: ") + api->GetErrorString(r_));
    rc = launch_scatter(c, part, st);
    if (rc) return rc;
    rc = c->timing ? c->xtiming.end(st) : 0;
    if (rc) return rc;
    if (overlap) HIP_TRY(hipEventRecord(c->ev_scatter[part], c->comm_stream));
    return 0;
}

// one half-step of this device's whole share; with a communicator, followed by the exchange
int half_step_all(vamp_ctx* c, int half) {
    RoctxRange range(half ? "vamp half-step 1 (blue moves)" : "vamp half-step 0 (red moves)");
    for (int p = 0; p < c->shard_parts; ++p) {
        int rc = launch_half(c, half, false, 0, 0, p);
        if (rc) return rc;
        if (c->comm && c->exchange) {
            rc = exchange_part(c, p);
            if (rc) return rc;
        }
    }
    if (c->comm && c->exchange && c->shard_parts > 1)
        for (int p = 0; p < c->shard_parts; ++p) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_scatter[p], 0));
    return 0;
}

int free_comm(vamp_ctx* c) {
    if (c->rccl) {
        RcclApi* api = nullptr;
        if (rccl_api(&api) == 0) (void)api->CommDestroy(c->rccl);
        c->rccl = nullptr;
    }
    for (hipEvent_t e : c->ev_kernel) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_scatter) (void)hipEventDestroy(e);
    c->ev_kernel.clear();
    c->ev_scatter.clear();
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    c->comm_stream = nullptr;
    vamp::leave_comm(c);
    return 0;
}

}  // namespace

extern "C" {

// Test hook, not part of the header: the resident workgroups run_resident would launch for the sampler's W, one row of
// {class kind, compute wavefronts, walkers per round, dynamic LDS bytes} per launch class (at most max_classes rows).
// Returns the number of classes, or an error code.
long long vampdbg_resident_plan(vamp_ctx* c, int max_classes, long long* rows) {
    if (!c || !rows || max_classes < 0) return fail(VAMP_ERR_ARG, "vampdbg_resident_plan: bad argument");
    if (!c->sampler_ready) return fail(VAMP_ERR_STATE, "vampdbg_resident_plan: call vamp_sampler_init first");
    const long long halfW = c->W / 2;
    const std::vector<LaunchClass>& classes = partition_for(c, halfW);
    for (size_t ci = 0; ci < classes.size() && (int)ci < max_classes; ++ci) {
        const LaunchClass& cl = classes[ci];
        const int shape = launch_shape(c, cl, halfW);
        const int nw = resident_waves_for(c, shape, halfW);
        long long lds = 0;
        VAMP_FOR_MODE_PK(c->f32, c->mode, shape, lds = resident_lds<F32, M, PK>(nw));
        long long* row = rows + 4 * ci;
        row[0] = cl.kind;
        row[1] = nw;
        row[2] = (long long)nw * (shape_walkers_per_block(shape) / shape_waves(shape));
        row[3] = lds;
    }
    return (long long)classes.size();
}

// Test hook, not part of the header: the launches an entry point makes for `movers_per_region` movers per region (a W-walker
// ensemble: W / 2; W points of vamp_lnprob(_all): (W + 1) / 2; ignored by the MAP search, which asks with one).  entry 0:
// the sampler's half-step (and the resident loop), 1: vamp_lnprob_all, 2: vamp_lnprob(region), 3: the device MAP search.
// One row of {class kind, shape (enum Shape), walkers per workgroup, threads per workgroup, regions of the class} per launch
// class, at most max_classes rows; region >= 0: only the class of that region (entry 2 needs one).  Returns the number of
// rows, or an error code.
long long vampdbg_launch_plan(vamp_ctx* c, long long movers_per_region, int entry, int region, int max_classes, long long* rows) {
    if (!c || !rows || max_classes < 0 || entry < 0 || entry > 3 || movers_per_region < 1) return fail(VAMP_ERR_ARG, "vampdbg_launch_plan: bad argument");
    if (c->regions_h.empty()) return fail(VAMP_ERR_STATE, "vampdbg_launch_plan: call vamp_set_regions first");
    if (region >= c->n_regions || (entry == 2 && region < 0)) return fail(VAMP_ERR_ARG, "vampdbg_launch_plan: no such region");
    const long long per = entry == 3 ? MAP_MOVERS : movers_per_region;
    const std::vector<LaunchClass>& classes = partition_for(c, per);
    const std::vector<int>& class_of = class_of_for(c, per);
    long long n = 0;
    for (size_t ci = 0; ci < classes.size(); ++ci) {
        const LaunchClass& cl = classes[ci];
        if (region >= 0 && class_of[region] != (int)ci) continue;
        if (n < max_classes) {
            const int shape = launch_shape(c, cl, per);
            long long* row = rows + 5 * n;
            row[0] = cl.kind;
            row[1] = shape;
            row[2] = shape_walkers_per_block(shape);
            row[3] = shape_threads(shape);
            row[4] = (long long)cl.regions.size();
        }
        ++n;
    }
    return n;
}

// Test hook, not part of the header: the context's far-field tables (k_tile_tables) as vamp_set_regions left them.  With N
// the pixels of all regions: u_out [N] (fp64 contexts) or uf_out [N] (fp32 contexts; the other pointer is not touched),
// geo_out [2 (N / 256 + 1)] as (mid, +-half) pairs.  Host code only: three copies.  Returns the number of geo slots, 0
// when the context holds no tables (no full tile, or Gaussian lines), or an error code.
long long vampdbg_tile_tables(vamp_ctx* c, double* u_out, float* uf_out, double* geo_out) {
    if (!c || !geo_out || !(c->f32 ? (void*)uf_out : (void*)u_out)) return fail(VAMP_ERR_ARG, "vampdbg_tile_tables: bad argument");
    if (c->regions_h.empty()) return fail(VAMP_ERR_STATE, "vampdbg_tile_tables: call vamp_set_regions first");
    if (!c->geo_d) return 0;
    const long long N = c->regions_h.back().pix_off + c->regions_h.back().P;
    const long long slots = N / (64 * TPIX) + 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->f32) HIP_TRY(hipMemcpy(uf_out, c->uf_d.get(), N * sizeof(float), hipMemcpyDeviceToHost));
    else HIP_TRY(hipMemcpy(u_out, c->u_d.get(), N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(geo_out, c->geo_d.get(), slots * sizeof(double2), hipMemcpyDeviceToHost));
    return slots;
}

// Test hook, not part of the header: the tiles' records behind the moment form (k_tile_tables, ff_moments.hpp), slot by
// slot like geo: out [slots x doubles per tile].  With out == nullptr nothing is copied.  Returns the doubles per tile
// (FFN_TILE or FFM_TILE, as the library was built), 0 when the context holds no record, or an error code.
long long vampdbg_tile_moments(vamp_ctx* c, double* out) {
    if (!c) return fail(VAMP_ERR_ARG, "vampdbg_tile_moments: bad argument");
    if (c->regions_h.empty()) return fail(VAMP_ERR_STATE, "vampdbg_tile_moments: call vamp_set_regions first");
    if (!VAMP_TILE_MOMENTS || c->f32 || !c->geo_d || !c->mom_d) return 0;
    const long long N = c->regions_h.back().pix_off + c->regions_h.back().P;
    const long long slots = N / (64 * TPIX) + 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out) HIP_TRY(hipMemcpy(out, c->mom_d.get(), slots * MOM_TILE * sizeof(double), hipMemcpyDeviceToHost));
    return MOM_TILE;
}

// Test hook, not part of the header: the far-field node stage of every full tile of `region` at the parameter vector
// theta [D] (k_dbg_node_sums): nodes [tiles x 16] = the optical depth of the tile's far, mid and wide lines at its 16
// Chebyshev nodes, sets [tiles x 5] = {far, n6, n4, n3, wide} at the first tile of every batch the line-major pass took
// (ff_node_pass) and 0xffffffff elsewhere.  Returns the number of full tiles, 0 when the context runs no fp64 far field
// (fp32, Gaussian lines, no full tile, more than 16 lines), or an error code.
static long long dbg_node_sums(vamp_ctx* c, int region, const double* theta, double* nodes, unsigned* sets, bool adj) {
    if (!c || !theta || !nodes || !sets) return fail(VAMP_ERR_ARG, "vampdbg_node_sums: bad argument");
    if (c->regions_h.empty()) return fail(VAMP_ERR_STATE, "vampdbg_node_sums: call vamp_set_regions first");
    if (region < 0 || region >= c->n_regions) return fail(VAMP_ERR_ARG, "vampdbg_node_sums: no such region");
    const RegionDev& R = c->regions_h[region];
    const long long tiles = R.P / (64 * TPIX);
    if (c->f32 || c->mode == VAMP_GAUSS3 || !c->geo_d || tiles == 0 || R.K > KMAX) return 0;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<double> th_d, nodes_d;
    DevBuf<unsigned> sets_d;
    HIP_TRY(th_d.ensure(R.D));
    HIP_TRY(nodes_d.ensure(tiles * FF_NODES));
    HIP_TRY(sets_d.ensure(tiles * 5));
    HIP_TRY(hipMemcpy(th_d.get(), theta, R.D * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(nodes_d.get(), 0, tiles * FF_NODES * sizeof(double)));
    HIP_TRY(hipMemset(sets_d.get(), 0xff, tiles * 5 * sizeof(unsigned)));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->mode == VAMP_VOIGT4)
        hipLaunchKernelGGL((k_dbg_node_sums<VAMP_VOIGT4>), dim3(1), dim3(PackSplit::THREADS), 0, c->stream, c->regions_d.get(), region, c->pix(),
                           th_d.get(), nodes_d.get(), sets_d.get(), adj);
    else
        hipLaunchKernelGGL((k_dbg_node_sums<VAMP_NBZ3>), dim3(1), dim3(PackSplit::THREADS), 0, c->stream, c->regions_d.get(), region, c->pix(),
                           th_d.get(), nodes_d.get(), sets_d.get(), adj);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(nodes, nodes_d.get(), tiles * FF_NODES * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sets, sets_d.get(), tiles * 5 * sizeof(unsigned), hipMemcpyDeviceToHost));
    return tiles;
}
// 1 when the library was built with the distant pass (VAMP_SUPER_NODES and VAMP_DEAL_ADJ): what the hook below then runs
int vampdbg_super_nodes(void) { return VAMP_SUPER_ON; }
long long vampdbg_node_sums(vamp_ctx* c, int region, const double* theta, double* nodes, unsigned* sets) {
    return dbg_node_sums(c, region, theta, nodes, sets, false);
}
// ... with the batches as the loop deals them when it was built with VAMP_DEAL_ADJ: four adjacent tiles, the tiles past the
// last whole group of 16 through the tile-by-tile stage.  Returns 0 when the library was built without the switch.
long long vampdbg_node_sums_adj(vamp_ctx* c, int region, const double* theta, double* nodes, unsigned* sets) {
    if (!(VAMP_DEAL_ADJ && VAMP_NODE_PASS_ON)) return 0;
    return dbg_node_sums(c, region, theta, nodes, sets, true);
}

int vamp_version(void) { return VAMP_ABI_VERSION; }

const char* vamp_last_error(void) { return vamp::last_error().c_str(); }

int vamp_device_count(int* n) {
    if (int rc = vamp::check_device_count(n)) return rc;
    HIP_TRY(hipGetDeviceCount(n));
    return VAMP_OK;
}

int vamp_ctx_create(vamp_ctx** out, int device, int dtype, int wofz_kind) {
    if (int rc = vamp::check_ctx_create(out, dtype, wofz_kind)) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (int rc = vamp::check_device(device, ndev)) return rc;
    HIP_TRY(hipSetDevice(device));
    vamp_ctx* c = nullptr;
    if (int rc = vamp::new_ctx(&c, dtype)) return rc;
    c->device = device;
    c->wofz_kind = wofz_kind;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(VAMP_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    c->stream = c->own_stream;
    if (const char* e = getenv("VAMP_CLASS_STREAMS")) c->concurrent_classes = std::atoi(e) != 0;
    if (const char* e = getenv("VAMP_RESIDENT")) c->opt_resident = std::max(0, std::min(2, std::atoi(e)));          // (A/B knobs of tools/ and profiles/;
    if (const char* e = getenv("VAMP_MAP_DEVICE")) c->opt_map_device = std::atoi(e) != 0;      //  vamp_ctx_set_option overrides them)
    *out = c;
    return VAMP_OK;
}

int vamp_ctx_destroy(vamp_ctx* c) {
    if (!c) return VAMP_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    free_comm(c);
    for (hipStream_t st : c->cls_stream) (void)hipStreamDestroy(st);
    for (hipEvent_t e : c->ev_join) (void)hipEventDestroy(e);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                  // (its memory and timing events with it)
    return VAMP_OK;
}

int vamp_ctx_set_stream(vamp_ctx* c, void* hip_stream) {
    if (int rc = vamp::need_ctx(c, "vamp_ctx_set_stream")) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return VAMP_OK;
}

int vamp_ctx_set_stream_default(vamp_ctx* c) {
    if (int rc = vamp::need_ctx(c, "vamp_ctx_set_stream_default")) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = nullptr;       // HIP's legacy default stream: what callers that never create a stream run on
    return VAMP_OK;
}

int vamp_ctx_set_packing(vamp_ctx* c, int lanes_per_walker) { return vamp::set_packing(c, lanes_per_walker); }

int vamp_ctx_set_option(vamp_ctx* c, const char* name, int64_t value) {
    if (int rc = vamp::check_option(c, name)) return rc;
    const std::string key(name);
    if (key == "map_device") c->opt_map_device = value != 0;
    else if (key == "resident") c->opt_resident = value < 0 ? 0 : value > 2 ? 2 : (int)value;
    else c->concurrent_classes = value != 0;
    return VAMP_OK;
}

int vamp_ctx_synchronize(vamp_ctx* c) {
    if (int rc = vamp::need_ctx(c, "vamp_ctx_synchronize")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VAMP_OK;
}

int vamp_set_regions(vamp_ctx* c, int n_regions, const int64_t* pix_off, const double* x, const double* flux,
                     const double* noise, const int32_t* n_comp, int mode, int sample_sd, int include_norm,
                     const double* bounds, const double* nbz) {
    if (int rc = vamp::check_set_regions(c, n_regions, pix_off, x, flux, noise, n_comp, mode, nbz)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    reset_sampler(c);
    reset_regions(c);
    static_assert(KMAX == 16 && KMAX_ALL == 32 && PackSmall::KCAP == 8 && PackSmall2::KCAP == 2 && VAMP_MID_MIN_K == 3 &&
                  VAMP_MID_MIN_P == 96 && BLEND_MAX_PIXELS == 512 && 64 * TPIX == 256, "vamp::plan::Limits describes these shapes");
    if (int rc = vamp::build_regions(c, n_regions, pix_off, x, noise, n_comp, mode, sample_sd, include_norm, bounds, nbz, VAMP_F32_TABLES != 0))
        return rc;
    const std::vector<RegionDev>& R = c->regions_h;
    const long long N = pix_off[n_regions];
    const std::vector<double> wt = vamp::pixel_weights(N, noise, sample_sd);
    HIP_TRY(c->x_d.ensure(N));
    HIP_TRY(c->f_d.ensure(N));
    HIP_TRY(c->wt_d.ensure(N));
    HIP_TRY(hipMemcpy(c->x_d.get(), x, N * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->f_d.get(), flux, N * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->wt_d.get(), wt.data(), N * sizeof(double), hipMemcpyHostToDevice));
    if (c->f32) {
        std::vector<float> t(N);
        HIP_TRY(c->xf_d.ensure(N));
        HIP_TRY(c->ff_d.ensure(N));
        HIP_TRY(c->wtf_d.ensure(N));
        for (long long i = 0; i < N; ++i) t[i] = (float)x[i];
        HIP_TRY(hipMemcpy(c->xf_d.get(), t.data(), N * sizeof(float), hipMemcpyHostToDevice));
        for (long long i = 0; i < N; ++i) t[i] = (float)flux[i];
        HIP_TRY(hipMemcpy(c->ff_d.get(), t.data(), N * sizeof(float), hipMemcpyHostToDevice));
        for (long long i = 0; i < N; ++i) t[i] = (float)wt[i];
        HIP_TRY(hipMemcpy(c->wtf_d.get(), t.data(), N * sizeof(float), hipMemcpyHostToDevice));
    }
    HIP_TRY(c->regions_d.ensure(n_regions));
    HIP_TRY(hipMemcpy(c->regions_d.get(), R.data(), n_regions * sizeof(RegionDev), hipMemcpyHostToDevice));
    // far-field tables (k_tile_tables), where a sweep can read them: Voigt lines and some region with a full tile
    int max_tiles = 0;
    bool any_full = false;
    for (const RegionDev& d : R) {
        max_tiles = std::max(max_tiles, (d.P + 64 * TPIX - 1) / (64 * TPIX));
        any_full = any_full || d.P >= 64 * TPIX;
    }
    if (mode != VAMP_GAUSS3 && any_full) {
        if (c->f32) HIP_TRY(c->uf_d.ensure(N));
        else HIP_TRY(c->u_d.ensure(N));
        HIP_TRY(c->geo_d.ensure(N / (64 * TPIX) + 1));
        if (VAMP_TILE_MOMENTS && !c->f32) {       // (cleared: a slot without a full tile holds no record, vampdbg_tile_moments shows it)
            HIP_TRY(c->mom_d.ensure((N / (64 * TPIX) + 1) * MOM_TILE));
            HIP_TRY(hipMemsetAsync(c->mom_d.get(), 0, (N / (64 * TPIX) + 1) * MOM_TILE * sizeof(double), c->stream));
        }
        VAMP_FOR_F32(c->f32, hipLaunchKernelGGL((k_tile_tables<F32>), dim3((unsigned)max_tiles, (unsigned)n_regions), dim3(64 * TPIX), 0,
                                                c->stream, c->regions_d.get(), c->x_d.get(), c->xf_d.get(), c->u_d.get(),
                                                c->uf_d.get(), c->geo_d.get(), c->f_d.get(), c->wt_d.get(), c->mom_d.get()));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));      // (the stream may be exchanged before the first sweep)
    }
    // the launch classes of both partitions, with their region lists on the device
    for (int which = 0; which < 2; ++which) {
        const vamp::plan::ClassPlan& pl = which ? c->plan_small : c->plan;
        std::vector<LaunchClass>& part = which ? c->classes_small : c->classes;
        for (size_t k = 0; k < pl.kind.size(); ++k) part.push_back(LaunchClass{pl.kind[k], pl.regions[k]});
#if VAMP_LPT
        // small ensembles: a launch is a few rounds of wavefronts, each a serial chain whose length grows with the region's
        // lines x pixels; the longest chains go FIRST, so that none starts in the last round (regions are independent and the
        // draws are keyed by region and walker: the order changes no result)
        bool reordered = false;
        if (which == 1 || VAMP_LPT == 2)
            for (LaunchClass& cl : part) {
                std::vector<int> before = cl.regions;
                std::stable_sort(cl.regions.begin(), cl.regions.end(), [&](int a, int b) {
                    return (long long)R[a].K * R[a].P > (long long)R[b].K * R[b].P;
                });
                reordered = reordered || before != cl.regions;
            }
        if (part.size() > 1 || reordered)
#else
        if (part.size() > 1)
#endif
            for (LaunchClass& cl : part) {
                HIP_TRY(cl.list_d.ensure(cl.regions.size()));
                HIP_TRY(hipMemcpy(cl.list_d.get(), cl.regions.data(), cl.regions.size() * sizeof(int), hipMemcpyHostToDevice));
            }
    }
    c->n_regions = n_regions;
    c->n_pix = N;
    return VAMP_OK;
}

int vamp_set_region_ids(vamp_ctx* c, const int32_t* ids) {
    if (int rc = vamp::set_region_ids(c, ids)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->regions_d.get(), c->regions_h.data(), c->n_regions * sizeof(RegionDev), hipMemcpyHostToDevice));
    return VAMP_OK;
}

int vamp_region_class(vamp_ctx* c, int region, int* kind, int* n_classes) { return vamp::region_class(c, region, kind, n_classes); }

int vamp_region_ndim(vamp_ctx* c, int region, int* ndim) { return vamp::region_ndim(c, region, ndim); }

namespace {
// k_lnprob on device arrays: region >= 0: theta[W, D] of that region -> lnprob[W]; region < 0: every
// region, theta = the regions' [W, D_r] blocks one after the other -> lnprob[n_regions, W]; one launch
// per launch class (blockIdx.y walks the class's region list)
int launch_lnprob(vamp_ctx* c, int region, long long W, const double* th_d, double* lp_d, double* ch_d) {
    const bool all = region < 0;
    // (one region per block row: every wave lies inside one region, so every class may pack)
    const long long per = lnprob_movers(W);
    const std::vector<LaunchClass>& classes = partition_for(c, per);
    const std::vector<int>& class_of = class_of_for(c, per);
    for (size_t ci = 0; ci < classes.size(); ++ci) {
        const LaunchClass& cl = classes[ci];
        if (!all && class_of[region] != (int)ci) continue;
        // the class's movers are counted as the sampler counts them, for one region too: a point has the same lnprob
        // bits through vamp_lnprob(region), vamp_lnprob_all and the sampler that steps it
        const int shape = launch_shape(c, cl, per);
        const long long per_block = shape_walkers_per_block(shape);
        const dim3 grid((unsigned)((W + per_block - 1) / per_block), all ? (unsigned)cl.regions.size() : 1u);
        const dim3 threads(shape_threads(shape));
        VAMP_FOR_MODE_PK(c->f32, c->mode, shape, hipLaunchKernelGGL((k_lnprob<F32, M, PK>), grid, threads, 0, c->stream, c->regions_d.get(), region,
                                                                c->pix(), W, th_d, lp_d, ch_d, (const int*)cl.list_d.get()));
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

constexpr size_t PINNED_EVAL_BYTES = 1u << 20;     // parameter blocks up to 1 MB are read by the kernel from pinned host memory
// region >= 0: W parameter vectors of that region; region < 0: W vectors of EVERY region
int lnprob_impl(vamp_ctx* c, int region, int64_t W, const double* theta, double* lnprob, double* chi2) {
    HIP_TRY(hipSetDevice(c->device));
    const bool all = region < 0;
    const long long dsum = all ? c->regions_h.back().d_before + c->regions_h.back().D : c->regions_h[region].D;
    const size_t nth = (size_t)W * dsum;
    const size_t nout = (size_t)W * (all ? c->n_regions : 1);
    if (nth * sizeof(double) <= PINNED_EVAL_BYTES) {
        HIP_TRY(c->pin_th.ensure(std::max(nth, (size_t)4096)));
        HIP_TRY(c->pin_out.ensure(std::max(2 * nout, (size_t)1024)));
        std::memcpy(c->pin_th.get(), theta, nth * sizeof(double));
        double* lp_h = c->pin_out.get();
        double* ch_h = chi2 ? lp_h + nout : nullptr;
        int rc = launch_lnprob(c, region, W, c->pin_th.get(), lp_h, ch_h);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::memcpy(lnprob, lp_h, nout * sizeof(double));
        if (chi2) std::memcpy(chi2, ch_h, nout * sizeof(double));
        return VAMP_OK;
    }
    HIP_TRY(c->sc_th.ensure(nth));
    HIP_TRY(c->sc_lp.ensure(nout));
    HIP_TRY(c->sc_chi.ensure(nout));
    double *th_d = c->sc_th.get(), *lp_d = c->sc_lp.get(), *ch_d = chi2 ? c->sc_chi.get() : nullptr;
    HIP_TRY(hipMemcpyAsync(th_d, theta, nth * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int rc = launch_lnprob(c, region, W, th_d, lp_d, ch_d);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(lnprob, lp_d, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (chi2) HIP_TRY(hipMemcpyAsync(chi2, ch_d, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VAMP_OK;
}
}  // namespace

int vamp_lnprob(vamp_ctx* c, int region, int64_t W, const double* theta, double* lnprob, double* chi2) {
    if (int rc = vamp::check_lnprob(c, region, W, theta, lnprob)) return rc;
    return lnprob_impl(c, region, W, theta, lnprob, chi2);
}

int vamp_lnprob_all(vamp_ctx* c, int64_t W, const double* theta, double* lnprob, double* chi2) {
    if (int rc = vamp::check_lnprob_all(c, W, theta, lnprob)) return rc;
    RoctxRange range("vamp_lnprob_all");
    return lnprob_impl(c, -1, W, theta, lnprob, chi2);
}

int vamp_map_all(vamp_ctx* c, const double* theta0, const uint8_t* active, int64_t maxiter, int64_t maxfun, double xtol,
                 double ftol, double* theta_best, double* lnprob_best, double* chi2_best, int64_t* iterations) {
    if (int rc = vamp::check_map_all(c, theta0, maxiter, maxfun, xtol, ftol, theta_best, lnprob_best)) return rc;
    RoctxRange range("vamp_map_all");
    if (c->opt_map_device) {
        // every region's whole search in ONE launch per launch class (k_map_search), no per-iteration synchronisation
        HIP_TRY(hipSetDevice(c->device));
        const RegionDev& last = c->regions_h.back();
        const size_t nth = (size_t)(last.d_before + last.D), nsim = (size_t)(last.sim_off + (long long)(last.D + 1) * last.D);
        const size_t nr = (size_t)c->n_regions;
        HIP_TRY(c->map_th_d.ensure(nth));
        HIP_TRY(c->map_best_d.ensure(nth));
        HIP_TRY(c->map_sim_d.ensure(nsim));
        HIP_TRY(c->map_act_d.ensure(nr));
        HIP_TRY(c->map_it_d.ensure(nr));
        HIP_TRY(hipMemcpyAsync(c->map_th_d.get(), theta0, nth * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (active) HIP_TRY(hipMemcpyAsync(c->map_act_d.get(), active, nr, hipMemcpyHostToDevice, c->stream));
        const unsigned char* act_d = active ? c->map_act_d.get() : nullptr;
        const std::vector<LaunchClass>& classes = partition_for(c, MAP_MOVERS);
        for (size_t ci = 0; ci < classes.size(); ++ci) {
            const LaunchClass& cl = classes[ci];
            // the shape vamp_lnprob runs a single point of this class in: the objective has the same bits
            const int shape = launch_shape(c, cl, MAP_MOVERS);
            const dim3 grid((unsigned)cl.regions.size()), threads(shape_threads(shape));
            VAMP_FOR_MODE_PK(c->f32, c->mode, shape, hipLaunchKernelGGL((k_map_search<F32, M, PK>), grid, threads, 0, c->stream, c->regions_d.get(),
                                                                    c->pix(), (const int*)cl.list_d.get(), c->map_th_d.get(), act_d, (long long)maxiter,
                                                                    (long long)maxfun, xtol, ftol, c->map_sim_d.get(), c->map_best_d.get(),
                                                                    c->map_it_d.get()));
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(theta_best, c->map_best_d.get(), nth * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        std::vector<long long> its(iterations ? nr : 0);
        if (iterations) HIP_TRY(hipMemcpyAsync(its.data(), c->map_it_d.get(), nr * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (iterations) for (size_t r = 0; r < nr; ++r) iterations[r] = its[r];
        return lnprob_impl(c, -1, 1, theta_best, lnprob_best, chi2_best);
    }
    // the host-driven form (vamp_ctx_set_option "map_device" = 0): csrc/map_search.hpp (scipy fmin's rules; shared with
    // the host build of this ABI), one launch + one synchronisation per iteration of all regions
    int rc = vamp::map_search_host(c, theta0, active, maxiter, maxfun, xtol, ftol, theta_best, iterations,
                                   [&](int W, const double* th, double* lp) { return lnprob_impl(c, -1, W, th, lp, nullptr); });
    if (rc) return rc;
    return lnprob_impl(c, -1, 1, theta_best, lnprob_best, chi2_best);
}

int vamp_model(vamp_ctx* c, int region, const double* theta1, double* tau_comp, double* flux_model) {
    if (int rc = vamp::check_model(c, "vamp_model", region, theta1)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const RegionDev& R = c->regions_h[region];
    DevBuf<double> th_d, tau_d, fl_d;
    HIP_TRY(th_d.ensure(R.D));
    if (tau_comp) HIP_TRY(tau_d.ensure((size_t)R.K * R.P));
    if (flux_model) HIP_TRY(fl_d.ensure(R.P));
    HIP_TRY(hipMemcpyAsync(th_d.get(), theta1, R.D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const unsigned grid = (unsigned)((R.P + BLOCK - 1) / BLOCK);
    VAMP_FOR_MODE(c->mode, hipLaunchKernelGGL((k_model<M>), dim3(grid), dim3(BLOCK), 0, c->stream, c->regions_d.get(), region, c->pix(),
                                              th_d.get(), tau_d.get(), fl_d.get()));
    HIP_TRY(hipGetLastError());
    if (tau_comp) HIP_TRY(hipMemcpyAsync(tau_comp, tau_d.get(), (size_t)R.K * R.P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (flux_model) HIP_TRY(hipMemcpyAsync(flux_model, fl_d.get(), (size_t)R.P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VAMP_OK;
}

int vamp_model_all(vamp_ctx* c, const double* theta, double* tau_comp, double* flux_model) {
    if (int rc = vamp::check_model_all(c, theta)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const RegionDev& last = c->regions_h.back();
    const size_t nth = (size_t)(last.d_before + last.D), ntau = (size_t)(last.tau_off + (long long)last.K * last.P);
    int pmax = 0;
    for (const RegionDev& R : c->regions_h) pmax = std::max(pmax, R.P);
    DevBuf<double> th_d, tau_d, fl_d;
    HIP_TRY(th_d.ensure(nth));
    if (tau_comp) HIP_TRY(tau_d.ensure(ntau));
    if (flux_model) HIP_TRY(fl_d.ensure(c->n_pix));
    HIP_TRY(hipMemcpyAsync(th_d.get(), theta, nth * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const dim3 grid((unsigned)((pmax + BLOCK - 1) / BLOCK), (unsigned)c->n_regions);
    VAMP_FOR_MODE(c->mode, hipLaunchKernelGGL((k_model<M>), grid, dim3(BLOCK), 0, c->stream, c->regions_d.get(), -1, c->pix(), th_d.get(),
                                              tau_d.get(), fl_d.get()));
    HIP_TRY(hipGetLastError());
    if (tau_comp) HIP_TRY(hipMemcpyAsync(tau_comp, tau_d.get(), ntau * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (flux_model) HIP_TRY(hipMemcpyAsync(flux_model, fl_d.get(), (size_t)c->n_pix * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VAMP_OK;
}

int vamp_line_records(vamp_ctx* c, int region, const double* theta1, double* rec, double* lnprior) {
    if (int rc = vamp::check_model(c, "vamp_line_records", region, theta1 && rec && lnprior)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const RegionDev& R = c->regions_h[region];
    DevBuf<double> th_d, rec_d;
    HIP_TRY(th_d.ensure(R.D));
    HIP_TRY(rec_d.ensure(5 * R.K + 1));
    HIP_TRY(hipMemcpyAsync(th_d.get(), theta1, R.D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    VAMP_FOR_MODE(c->mode, hipLaunchKernelGGL((k_line_records<M>), dim3(1), dim3(64), 0, c->stream, c->regions_d.get(), region, th_d.get(),
                                              rec_d.get(), rec_d.get() + 5 * R.K));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rec, rec_d.get(), 5 * R.K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(lnprior, rec_d.get() + 5 * R.K, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VAMP_OK;
}

int vamp_wofz_re(vamp_ctx* c, int64_t n, const double* x, const double* y, double* re_w) {
    if (int rc = vamp::check_wofz(c, n, x, y, re_w)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<double> x_d, y_d, o_d;
    HIP_TRY(x_d.ensure(n));
    HIP_TRY(y_d.ensure(n));
    HIP_TRY(o_d.ensure(n));
    HIP_TRY(hipMemcpyAsync(x_d.get(), x, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(y_d.get(), y, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    VAMP_FOR_F32(c->f32, hipLaunchKernelGGL((k_wofz<F32>), dim3(grid), dim3(BLOCK), 0, c->stream, (long long)n, x_d.get(), y_d.get(), o_d.get()));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(re_w, o_d.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VAMP_OK;
}

int vamp_sampler_bind_state(vamp_ctx* c, void* X_dev, void* lnp_dev) {
    if (int rc = vamp::check_bind_state(c, X_dev, lnp_dev)) return rc;
    reset_sampler(c);
    c->X_d = (double*)X_dev;
    c->lnp_d = (double*)lnp_dev;
    return VAMP_OK;
}

int vamp_sampler_init(vamp_ctx* c, int64_t W, const double* theta0, uint64_t seed, double a, int32_t split_block) {
    if (int rc = vamp::check_sampler_init(c, W, theta0, a, split_block)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("vamp_sampler_init");
    HIP_TRY(hipStreamSynchronize(c->stream));
    vamp::init_sampler(c, W, seed, a, split_block);
    HIP_TRY(hipMemcpy(c->regions_d.get(), c->regions_h.data(), c->n_regions * sizeof(RegionDev), hipMemcpyHostToDevice));
    const bool bound = c->X_d && c->X_d != c->X_own.get();      // the caller's state (vamp_sampler_bind_state) is kept
    if (!bound) reset_sampler(c);
    c->nacc_d.reset();
    const long long tt = c->total_theta;
    if (!bound) {
        HIP_TRY(c->X_own.ensure(tt));
        HIP_TRY(c->lnp_own.ensure(c->total_walkers));
        c->X_d = c->X_own.get();
        c->lnp_d = c->lnp_own.get();
    }
    HIP_TRY(c->nacc_d.ensure(c->total_walkers));
    HIP_TRY(hipMemsetAsync(c->nacc_d.get(), 0, c->total_walkers * sizeof(long long), c->stream));
    HIP_TRY(hipMemcpyAsync(c->X_d, theta0, tt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // initial log-posteriors of every walker: the state has the layout of vamp_lnprob_all's arguments
    // (block r at W * d_before(r), lnprob of region r at r * W), so this is one launch per launch class
    {
        int rc = launch_lnprob(c, -1, W, c->X_d, c->lnp_d, nullptr);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sampler_ready = true;
    return VAMP_OK;
}

int vamp_sampler_set_shard_parts(vamp_ctx* c, int rank, int world, int parts, int64_t* own_begin, int64_t* own_end) {
    if (int rc = vamp::set_shard_parts(c, rank, world, parts, own_begin, own_end)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->send_d.reset();
    c->recv_d.reset();
    return vamp::needs_exchange(c) ? alloc_exchange_buffers(c) : VAMP_OK;
}

int vamp_sampler_set_shard(vamp_ctx* c, int rank, int world, int64_t* own_begin, int64_t* own_end) {
    return vamp_sampler_set_shard_parts(c, rank, world, 1, own_begin, own_end);
}

int vamp_sampler_state_ptrs(vamp_ctx* c, void** X_dev, void** lnp_dev, int64_t* total_theta, int64_t* total_walkers) {
    if (int rc = vamp::need_sampler(c, "vamp_sampler_state_ptrs")) return rc;
    if (X_dev) *X_dev = c->X_d;
    if (lnp_dev) *lnp_dev = c->lnp_d;
    if (total_theta) *total_theta = c->total_theta;
    if (total_walkers) *total_walkers = c->total_walkers;
    return VAMP_OK;
}

int vamp_sampler_half_step(vamp_ctx* c, int half) {
    if (int rc = vamp::check_half_step(c, half)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int rc = half_step_all(c, half);
    if (rc) return rc;
    if (half == 1) c->step += 1;
    return VAMP_OK;
}

int vamp_sampler_half_step_part(vamp_ctx* c, int half, int part) {
    if (int rc = vamp::check_half_step_part(c, half, part)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int rc = launch_half(c, half, false, 0, 0, part);
    if (rc) return rc;
    if (half == 1 && part == c->shard_parts - 1) c->step += 1;
    return VAMP_OK;
}

int vamp_sampler_half_step_ext(vamp_ctx* c, int region, int64_t n, const int32_t* active_idx, const int32_t* partner_idx,
                               const double* zz, const double* logu) {
    if (int rc = vamp::check_half_step_ext(c, region, n, active_idx, partner_idx, zz, logu)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->ext_act_d.ensure(n));
    HIP_TRY(c->ext_par_d.ensure(n));
    HIP_TRY(c->ext_z_d.ensure(n));
    HIP_TRY(c->ext_lu_d.ensure(n));
    HIP_TRY(hipMemcpyAsync(c->ext_act_d.get(), active_idx, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ext_par_d.get(), partner_idx, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ext_z_d.get(), zz, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ext_lu_d.get(), logu, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int rc = launch_half(c, 0, true, region, n);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VAMP_OK;
}

int vamp_sampler_run_dev(vamp_ctx* c, int64_t n_steps, int thin, double* chain_dev, double* lnprob_chain_dev, double* seconds) {
    if (int rc = vamp::check_run(c, true, n_steps, thin)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    RoctxRange range("vamp_sampler_run");
    const long long n_keep = n_steps / thin;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    long long kept = 0;
    if (n_steps > 0 && resident_eligible(c)) {
        // small ensembles: every region's whole step loop in ONE launch per launch class (k_run_resident)
        RoctxRange res_range("vamp resident step loop");
        int rc = run_resident(c, n_steps, thin, n_keep ? chain_dev : nullptr, n_keep ? lnprob_chain_dev : nullptr);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return VAMP_OK;
    }
    for (long long it = 0; it < n_steps; ++it) {
        for (int half = 0; half < 2; ++half) {
            int rc = half_step_all(c, half);
            if (rc) return rc;
        }
        c->step += 1;
        if ((it + 1) % thin == 0 && kept < n_keep) {
            if (chain_dev)
                HIP_TRY(hipMemcpyAsync(chain_dev + kept * c->total_theta, c->X_d, c->total_theta * sizeof(double),
                                       hipMemcpyDeviceToDevice, c->stream));
            if (lnprob_chain_dev)
                HIP_TRY(hipMemcpyAsync(lnprob_chain_dev + kept * c->total_walkers, c->lnp_d, c->total_walkers * sizeof(double),
                                       hipMemcpyDeviceToDevice, c->stream));
            ++kept;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    const auto t1 = std::chrono::steady_clock::now();
    if (seconds) *seconds = std::chrono::duration<double>(t1 - t0).count();
    return VAMP_OK;
}

int vamp_sampler_run(vamp_ctx* c, int64_t n_steps, int thin, double* chain, double* lnprob_chain, int64_t* n_accept,
                     double* seconds) {
    if (int rc = vamp::check_run(c, false, n_steps, thin)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const long long n_keep = n_steps / thin;
    DevBuf<double> chain_d, lchain_d;
    if (chain && n_keep) HIP_TRY(chain_d.ensure((size_t)n_keep * c->total_theta));
    if (lnprob_chain && n_keep) HIP_TRY(lchain_d.ensure((size_t)n_keep * c->total_walkers));
    int rc = vamp_sampler_run_dev(c, n_steps, thin, chain_d.get(), lchain_d.get(), seconds);
    if (rc) return rc;
    if (chain_d) HIP_TRY(hipMemcpy(chain, chain_d.get(), (size_t)n_keep * c->total_theta * sizeof(double), hipMemcpyDeviceToHost));
    if (lchain_d) HIP_TRY(hipMemcpy(lnprob_chain, lchain_d.get(), (size_t)n_keep * c->total_walkers * sizeof(double), hipMemcpyDeviceToHost));
    if (n_accept) HIP_TRY(hipMemcpy(n_accept, c->nacc_d.get(), c->total_walkers * sizeof(long long), hipMemcpyDeviceToHost));
    return VAMP_OK;
}

// ---- walker-sharded multi-GPU runs ------------------------------------------------------------
int vamp_comm_unique_id(char* id) {
    if (int rc = vamp::check_unique_id(id)) return rc;
    RcclApi* api = nullptr;
    int rc = rccl_api(&api);
    if (rc) return rc;
    RcclUniqueId u;
    RCCL_TRY(api, api->GetUniqueId(&u));
    std::memcpy(id, u.internal, VAMP_COMM_ID_BYTES);
    return VAMP_OK;
}

int vamp_comm_init_rank(vamp_ctx* c, const char* id, int rank, int world) {
    if (int rc = vamp::check_comm_init_rank(c, id, rank, world)) return rc;
    RcclApi* api = nullptr;
    int rc = rccl_api(&api);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // RCCL checks the runtime's sticky last error during initialisation: one left behind by an earlier call of
    // anyone in this process (a failed allocation, a rejected argument) would surface as "unhandled cuda error"
    (void)hipGetLastError();
    RcclUniqueId u;
    std::memcpy(u.internal, id, VAMP_COMM_ID_BYTES);
    void* comm = nullptr;
    RCCL_TRY(api, api->CommInitRank(&comm, world, u, rank));
    c->rccl = comm;
    const bool shard_first = vamp::join_comm(c, rank, world);
    HIP_TRY(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    // the shard came first: its exchange buffers (a single-rank shard has none yet) and per-part events are due now
    if (shard_first) {
        if (!c->exchange) rc = alloc_exchange_buffers(c);
        else rc = ensure_part_events(c, c->shard_parts);
        if (rc) return rc;
    }
    return VAMP_OK;
}

int vamp_comm_info(vamp_ctx* c, int* rank, int* world, int* queried) {
    if (int rc = vamp::check_comm_info(c)) return rc;
    int r = c->comm_rank, w = c->comm_world, q = 0;
    RcclApi* api = nullptr;
    if (rccl_api(&api) == 0 && api->CommCount && api->CommUserRank) {
        int w2 = 0, r2 = 0;
        RCCL_TRY(api, api->CommCount(c->rccl, &w2));
        RCCL_TRY(api, api->CommUserRank(c->rccl, &r2));
        r = r2; w = w2; q = 1;
    }
    if (rank) *rank = r;
    if (world) *world = w;
    if (queried) *queried = q;
    return VAMP_OK;
}

int vamp_comm_library(char* path, int64_t capacity) {
    if (int rc = vamp::check_comm_library(path, capacity)) return rc;
    RcclApi* api = nullptr;
    int rc = rccl_api(&api);
    if (rc) return rc;
    Dl_info info;
    const char* name = (dladdr(reinterpret_cast<void*>(api->AllGather), &info) && info.dli_fname) ? info.dli_fname : "";
    std::snprintf(path, (size_t)capacity, "%s", name);
    return VAMP_OK;
}

int vamp_comm_destroy(vamp_ctx* c) {
    if (int rc = vamp::need_ctx(c, "vamp_comm_destroy")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->comm_stream) HIP_TRY(hipStreamSynchronize(c->comm_stream));
    free_comm(c);
    return VAMP_OK;
}

int vamp_sampler_pack_get(vamp_ctx* c, int part, double* rows) {
    if (int rc = vamp::check_exchange_rows(c, false, part, rows)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t n = vamp::part_doubles(c, false);
    HIP_TRY(hipMemcpy(rows, c->send_d.get() + (size_t)part * n, n * sizeof(double), hipMemcpyDeviceToHost));
    return VAMP_OK;
}

int vamp_sampler_scatter_put(vamp_ctx* c, int part, const double* rows_all) {
    if (int rc = vamp::check_exchange_rows(c, true, part, rows_all)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = vamp::part_doubles(c, true);
    HIP_TRY(hipMemcpyAsync(c->recv_d.get() + (size_t)part * n, rows_all, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int rc = launch_scatter(c, part, c->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VAMP_OK;
}

int vamp_sampler_get_state(vamp_ctx* c, double* theta, double* lnprob, int64_t* n_accept, int64_t* step) {
    if (int rc = vamp::need_sampler(c, "vamp_sampler_get_state")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (theta) HIP_TRY(hipMemcpy(theta, c->X_d, c->total_theta * sizeof(double), hipMemcpyDeviceToHost));
    if (lnprob) HIP_TRY(hipMemcpy(lnprob, c->lnp_d, c->total_walkers * sizeof(double), hipMemcpyDeviceToHost));
    if (n_accept) HIP_TRY(hipMemcpy(n_accept, c->nacc_d.get(), c->total_walkers * sizeof(long long), hipMemcpyDeviceToHost));
    if (step) *step = c->step;
    return VAMP_OK;
}

int vamp_sampler_set_state(vamp_ctx* c, const double* theta, const double* lnprob, int64_t step) {
    if (int rc = vamp::check_set_state(c, theta, lnprob, step)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->X_d, theta, c->total_theta * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->lnp_d, lnprob, c->total_walkers * sizeof(double), hipMemcpyHostToDevice));
    c->step = step;
    return VAMP_OK;
}

int vamp_exchange_timing(vamp_ctx* c, double* total_ms, int64_t* exchanges) {
    if (int rc = vamp::need_ctx(c, "vamp_exchange_timing")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int rc = c->xtiming.flush();
    if (rc) return rc;
    if (total_ms) *total_ms = c->xtiming.ms;
    if (exchanges) *exchanges = c->xtiming.n;
    c->xtiming.ms = 0.0;
    c->xtiming.n = 0;
    return VAMP_OK;
}

#ifdef VAMP_STAMPS
// timing-only builds: copy out and reset the (tag, clock) stamps; returns their number
int vamp_debug_stamps(unsigned long long* out, int cap) {
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_stamp_n), sizeof(n)) != hipSuccess) return -1;
    if ((int)n > cap) n = (unsigned)cap;
    if (n && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), (size_t)n * 2 * sizeof(unsigned long long)) != hipSuccess) return -1;
    const unsigned int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_n), &zero, sizeof(zero)) != hipSuccess) return -1;
    return (int)n;
}
#endif

int vamp_kernel_timing(vamp_ctx* c, int enable, double* total_ms, int64_t* launches) {
    if (int rc = vamp::need_ctx(c, "vamp_kernel_timing")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int rc = c->ktiming.flush();
    if (rc) return rc;
    rc = c->xtiming.flush();
    if (rc) return rc;
    if (total_ms) *total_ms = c->ktiming.ms;
    if (launches) *launches = c->ktiming.n;
    c->ktiming.ms = 0.0;
    c->ktiming.n = 0;
    c->timing = enable != 0;
    return VAMP_OK;
}

}  // extern "C"
