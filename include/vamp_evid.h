/* vamp_evid.h -- log-evidence ln Z of absorption regions from a tempered ensemble on the GPU (libvamp_evid.so).
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h), libvamp_diag.so (include/vamp_diag.h)
 * and libvamp_post.so (include/vamp_post.h); it shares no state with a vamp_ctx.  Definitions: DESIGN.md "Evidence".
 *
 * Input: G regions.  Region g has
 *   x[g], flux[g], noise[g]   n_pix[g] >= 1 pixels each (HOST memory, finite); x strictly monotonic in either direction,
 *                    noise > 0 (read only when sample_sd[g] = 0)
 *   n_comp[g] = K    lines, 1 <= K <= VAMP_EVID_MAX_COMPONENTS
 *   mode[g]          0 = GAUSS3 (A, c, sigma) or 1 = VOIGT4 (A, c, L_fwhm, G_fwhm) per line: the layouts of enum vamp_mode.
 *                    Mode 2 (NBZ3) is rejected.  q = 3 or 4 parameters per line.
 *   sample_sd[g]     1: the last parameter is the free sd ~ U(0, 1) of the likelihood.  D = q K + sample_sd.
 *   bounds[g]        {c_lo, c_hi, sigma_max, fwhm_max} as in vamp_set_regions, or NULL (the array, or one entry) to
 *                    derive them from x[g]: c in [min x, max x], sigma_max = (max x - min x) / 2,
 *                    fwhm_max = sigma_max 2 sqrt(2 ln 2).  An empty range (a region of one pixel without bounds) is an error.
 *   region_id[g]     >= 0: the region's identity in the draw keys; a region follows the same trajectory alone or in a batch.
 *                    region_id * n_temps + n_temps - 1 must fit 31 bits.
 *
 * ln pi(theta): A ~ A exp(-A), c ~ U(c_lo, c_hi), widths ~ U(0, max), sd ~ U(0, 1): the prior the sampler of libvamp_hip.so
 * samples.  ln L(theta): -1/2 chi^2 - 1/2 sum log(2 pi noise_i^2) for known noise (the normalisation is always
 * included), n_pix/2 log(1 / (2 pi sd^2)) - sum (f - m)^2 / (2 sd^2) for the free sd.  Outside the prior ln L is not evaluated
 * and the point is rejected; a ln L that is not finite rejects the point too.  A width of exactly 0 (sigma = 0, G_fwhm = 0)
 * lies on the edge of the prior's closed range and has no ln L: it is reported like a point outside the prior (ln pi = -inf,
 * ln L = NaN, not evaluated), wherever its centre lies; sd = 0 keeps its ln pi and has ln L = -inf.  L_fwhm = 0 is an ordinary
 * point: a line of no depth.  ln Z = log of the integral of pi L.
 *
 * Sampler: T = n_temps rungs per region, inverse temperatures betas[0] = 0 < ... < betas[T - 1] = 1 (NULL: the ladder of
 * vamp_evid_default_betas), W = walkers each.  Rung j samples pi L^beta_j with the red/blue stretch move of libvamp_hip.so
 * (scale a, one split block of W walkers, draws keyed by (seed, step, half, walker) with the sampler's region id
 * region_id * T + j).  start[g]: a [W][D] block (HOST) copied to every rung, or NULL (the array, or one entry) for W
 * prior draws per rung.  Every start point must lie inside the prior and have a finite ln L.  After every swap_every
 * steps, swap n = 0, 1, ... offers the pairs (j, j + 1) with j % 2 == n % 2: walker w of both rungs exchange
 * positions when log u < (beta_{j+1} - beta_j)(ln L_j - ln L_{j+1}).  The steps burn .. n_steps - 1 are kept:
 * n_keep = n_steps - burn >= 1.
 *
 * Output, host arrays in region order; any pointer may be NULL:
 *   lnZ[G]           the stepping-stone estimate, sum_j log mean exp((beta_{j+1} - beta_j) ln L) over rung j's kept samples
 *   lnZ_se[G]        its standard error: the sample standard deviation (n - 1) of the estimates of VAMP_EVID_BLOCKS
 *                    consecutive time blocks (block b: kept steps b n_keep / 8 .. (b + 1) n_keep / 8 - 1), over sqrt(8); NaN when n_keep < 8
 *   lnZ_ti[G]        thermodynamic integration, the trapezoid of mean ln L over beta (a diagnostic)
 *   mean_lnL, var_lnL [G][T]   mean and population variance of the kept ln L per rung
 *   move_accept[G][T]          accepted / offered stretch moves, all steps
 *   swap_accept[G][T - 1]      accepted / offered swaps of the pair (j, j + 1), all steps; NaN when none was offered
 *   chain[g], chain_lnl[g]     the beta = 1 rung's kept chain [n_keep][W][D] and ln L [n_keep][W] (the arrays or single
 *                    entries may be NULL); host memory, or device memory of `device` when chain_is_device = 1
 *   lnl_trace        [G][n_keep][T][W]: ln L of every kept (step, rung, walker), before the swap that follows the step
 *   swap_trace       [G][n_swaps][T - 1][W] bytes, n_swaps = (n_steps - 1) / swap_every: 1 = exchanged (0 for pairs not offered)
 *
 * Every function returns 0 on success and -1 on an error; vamp_evid_last_error() then says why.  Every argument is
 * checked before the first HIP call.  The caller's current HIP device is restored before return.  Arithmetic is fp64.
 */
#ifndef VAMP_EVID_H
#define VAMP_EVID_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_EVID_ABI_VERSION 1
#define VAMP_EVID_MAX_COMPONENTS 8
#define VAMP_EVID_MAX_WALKERS 256
#define VAMP_EVID_MAX_TEMPS 64
#define VAMP_EVID_BLOCKS 8

int vamp_evid_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_evid_last_error(void);

/* betas[j] = (j / (n_temps - 1))^(1 / 0.3), 2 <= n_temps <= VAMP_EVID_MAX_TEMPS (Xie et al. 2011); no device call */
int vamp_evid_default_betas(int n_temps, double* betas);

/* Test hook: ln L and ln pi of n parameter vectors theta[n][D] (HOST) of one region, by the device function the sampler
 * uses.  Outside the prior lnprior is -inf and lnlike NaN (not evaluated); a ln L that is not finite is returned as -inf. */
int vamp_evid_lnlike(int device, const double* x, const double* flux, const double* noise, int n_pix, int n_comp, int mode,
                     int sample_sd, const double* bounds, int n, const double* theta, double* lnlike, double* lnprior);

/* device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default stream. */
int vamp_evid_run(int device, void* hip_stream, int n_regions, const double* const* x, const double* const* flux,
                  const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                  const int32_t* sample_sd, const double* const* bounds, const int32_t* region_id, int n_temps,
                  const double* betas, int walkers, int n_steps, int burn, int swap_every, uint64_t seed, double a,
                  const double* const* start, double* lnZ, double* lnZ_se, double* lnZ_ti, double* mean_lnL, double* var_lnL,
                  double* move_accept, double* swap_accept, double* const* chain, double* const* chain_lnl, int chain_is_device,
                  double* lnl_trace, uint8_t* swap_trace);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_EVID_H */
