/* vamp_laplace.h -- Laplace importance sampling on the GPU (libvamp_laplace.so): S independent draws from a Gaussian
 * proposal N(centre, C C^T) per region, the exact log-posterior at each, Pareto-smoothed importance ratios; from them
 * ln Z with a standard error, posterior mean, standard deviation and covariance, and the Pareto khat that says whether
 * any of it may be trusted.  No chain: every sample is independent.
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h) and the other side libraries; it shares
 * no state with a vamp_ctx.  Definitions: below, and DESIGN.md section 16, "Laplace importance sampling".
 * Source: Vehtari, Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling"; Zhang & Stephens (2009),
 * Technometrics 51, 316; Salmon, Moraes, Dror & Shaw (SC'11) for Philox.
 *
 * Input: G groups (one region each).  Group g has
 *   x[g][n_pix[g]]       the abscissa (HOST memory, finite, strictly monotonic); P = n_pix[g] >= 1
 *   flux[g][n_pix[g]]    the data (HOST memory, finite)
 *   noise[g][n_pix[g]]   HOST memory, finite and > 0; NULL exactly when sample_sd[g] = 1
 *   n_comp[g] = K        lines, 1 <= K <= VAMP_LAPLACE_MAX_COMPONENTS
 *   mode[g]              0 = GAUSS3 (A, c, sigma) or 1 = VOIGT4 (A, c, L_fwhm, G_fwhm) per line.  Mode 2 (NBZ3) is rejected.
 *   sample_sd[g]         1: the vector's last entry is the free sd, the noise of every pixel.  D = q K + sample_sd <= 65.
 *   bounds[g]            {c_lo, c_hi, sigma_max, fwhm_max} (HOST), or NULL (also bounds itself) to derive them from x as
 *                        vamp_evid.h does: c in [min x, max x], sigma_max = (max x - min x) / 2, fwhm_max = sigma_max
 *                        2 sqrt(2 ln 2).  A region of one pixel needs bounds.
 *   region_id[g]         >= 0, below 2^31: the group's identity in the draw keys
 *   centre[g][D]         the proposal's mean (HOST, finite)
 *   chol[g][D][D]        the lower factor C of the proposal covariance Sigma = C C^T, row-major (HOST).  Only the lower
 *                        triangle is read.  The caller has already applied any inflation.
 * Per call: n_samples = S with 2 <= S <= VAMP_LAPLACE_MAX_SAMPLES, and seed.
 *
 * Draws, keyed so that a group gives the same bits alone or in any batch.  For sample s and pair j = 0 .. ceil(D / 2) - 1:
 *   (c0, c1, c2, c3) = philox4x32_10({s, j, 5, region_id}, seed lo, seed hi)          (5 = STREAM_NORMAL)
 *   u1 = 1 - u53(c0, c1) in (0, 1],  u2 = u53(c2, c3),  u53(hi, lo) = ((hi << 32 | lo) >> 11) 2^-53
 *   rho = sqrt(-2 log u1),  z_2j = rho cos(2 pi u2),  z_2j+1 = rho sin(2 pi u2); the last z of an odd D is dropped
 *   theta_d = centre_d + acc_d, acc_d the fma chain of C_de z_e over e = 0 .. d, ascending, from 0
 *   ln q = -1/2 sum_d z_d^2 (d ascending) - sum_d ln C_dd - (D / 2) ln 2 pi
 *
 * Target: ln pi and ln L exactly as vamp_evid.h defines them -- priors A e^-A on amplitudes, uniform centres and widths,
 * sd ~ U(0, 1); the normalisation of ln L always included; outside the prior ln L is not evaluated; a width of exactly 0
 * is outside; a ln L that is not finite rejects the point.  ln p = ln pi + ln L, or -inf for a rejected point.
 *   r_s = ln p_s - ln q_s
 *
 * Weights: the definitions of vamp_loo.h, word for word, on these r_s in place of -l_s, with n = S: the tail length
 * M = min(ceil(S / 5), m3) in integers, the cutoff, the Zhang-Stephens fit, the prior on k, the smoothed tail, the
 * truncation at 0 after r_max = max_s r_s was subtracted.  Two additions: exp(-inf) = 0; and if fewer than M + 1 of
 * the r_s are finite, khat = +inf and the raw ratios stand.
 *   lw_s   the truncated log weights, before normalisation
 *   w~_s   = exp(lw_s) / sum_s exp(lw_s)
 *
 * Per group:
 *   lnZ        r_max + log((1 / S) sum_s exp(r_s - r_max)): plain importance sampling; rejected draws count in S
 *   lnZ_se     sqrt(var(w) / S) / mean(w),  w_s = exp(r_s - r_max),  var with S - 1 in the denominator, two passes
 *   lnZ_psis   r_max + log((1 / S) sum_s exp(lw_s))
 *   khat       as above
 *   ess        1 / sum_s w~_s^2
 *   n_out      the number of rejected draws
 *   lnp_centre ln p at the centre (the one evaluation the plain Laplace estimate needs)
 *   mean[D]    sum_s w~_s theta_s
 *   cov[D][D]  sum_s w~_s (theta_sd - mean_d)(theta_se - mean_e): two passes; full symmetric, row-major
 *   sd[D]      sqrt(cov_dd)
 * Every floating-point sum over the samples is a per-thread fold in sample order plus a block reduction of fixed order.
 * A group's results do not depend on the rest of the call, on host or device outputs, or on the stream: bit for bit.
 *
 * status of a group (none is an error of the call):
 *   0  ok.  If all S draws are rejected: lnZ = -inf, n_out = S, lnp_centre as evaluated, every other per-group value
 *      and lw NaN.
 *   1  no proposal: a diagonal entry of chol that is not finite or <= 0, or a read entry (lower triangle, centre) that
 *      is not finite.  Every output of the group is NaN (n_out = 0), the per-sample outputs included.
 *   2  the centre is rejected by the target's own rule.  Every per-group output and lw are NaN (n_out = 0, lnp_centre
 *      = -inf); z, theta, lnp and lnq are what was drawn.
 *
 * Output, HOST arrays in group order; any pointer may be NULL:
 *   lnZ, lnZ_se, lnZ_psis, khat, ess, lnp_centre      G doubles;   n_out, status: G int32
 *   mean, sd                                          sum of D doubles
 *   cov                                               sum of D^2 doubles
 * Per-sample outputs: G pointers each (or NULL for none); an entry may be NULL
 *   theta[g], z[g]        [S][D]; DEVICE memory if samples_are_device = 1, else HOST
 *   lnp[g], lnq[g], lw[g] [S], HOST
 *
 * Every function returns 0 on success and -1 on an error; vamp_laplace_last_error() then says why.  Every argument is
 * checked before the first HIP call.  The caller's current HIP device is restored before return.  Everything is fp64.
 */
#ifndef VAMP_LAPLACE_H
#define VAMP_LAPLACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_LAPLACE_ABI_VERSION 1
#define VAMP_LAPLACE_MAX_SAMPLES 16384
#define VAMP_LAPLACE_MAX_COMPONENTS 16
#define VAMP_LAPLACE_MAX_DIM 65                           /* 4 * 16 + 1 */
#define VAMP_LAPLACE_MAX_THETA_DOUBLES (1LL << 28)        /* sum of S D over the groups: 2 GiB of draws */

int vamp_laplace_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_laplace_last_error(void);

/* device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default stream. */
int vamp_laplace_points(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                        const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                        const int32_t* sample_sd, const double* const* bounds, const int32_t* region_id,
                        const double* const* centre, const double* const* chol, int n_samples, uint64_t seed, double* lnZ,
                        double* lnZ_se, double* lnZ_psis, double* khat, double* ess, double* lnp_centre, int32_t* n_out,
                        int32_t* status, double* mean, double* sd, double* cov, double* const* theta, double* const* z,
                        int samples_are_device, double* const* lnp, double* const* lnq, double* const* lw);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_LAPLACE_H */
