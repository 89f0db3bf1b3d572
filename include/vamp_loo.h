/* vamp_loo.h -- Pareto-smoothed importance-sampling leave-one-out predictive density (PSIS-LOO) of ensemble chains on
 * the GPU (libvamp_loo.so).
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h), libvamp_diag.so (include/vamp_diag.h),
 * libvamp_post.so (include/vamp_post.h), libvamp_evid.so (include/vamp_evid.h) and libvamp_pred.so
 * (include/vamp_pred.h): it reads chains wherever they are -- host arrays, or the device chain vamp_sampler_run_dev
 * wrote -- or log-likelihood matrices the caller already has, and shares no state with a vamp_ctx.
 * Definitions: below, and word for word in DESIGN.md "PSIS-LOO: leave-one-out predictive density per pixel".
 * Source: Vehtari, Gelman & Gabry (2017), Statistics and Computing 27, 1413; Vehtari, Simpson, Gelman, Yao & Gabry,
 * "Pareto smoothed importance sampling"; Zhang & Stephens (2009), Technometrics 51, 316.
 *
 * Input of vamp_loo_pointwise: the G groups, chains and data of vamp_pred_pointwise (include/vamp_pred.h), with its
 * layout, its limits and its rule of BAD samples, which are left out and counted.  l_sp is vamp_pred.h's
 * log-likelihood of pixel p's datum under sample s.
 *
 * Definitions.
 * For one pixel, let l_s be its log-likelihood over the n good samples, in sample order.
 *   Log ratios.    r_s = -l_s - max_s(-l_s).
 *   Tail length,   in integers so that no rounding can differ.  M = min(ceil(n / 5), m3), where m3 is the smallest
 *                  integer with m3^2 >= 9 n (3 sqrt(n): the relative efficiency of the draws is taken as 1).  M = 4 at
 *                  n = 20, 5 at n = 21, 384 at n = 16 384; the two terms cross between n = 225 and n = 231.
 *   No smoothing.  If M < 5, khat = +inf and the raw r are the log weights.
 *   Tail and cutoff.  Otherwise sort ascending by (value, sample index).  The tail is the last M samples.  The cutoff c
 *                  is the largest value not in the tail.  x_i = exp(r_tail,i) - exp(c), ascending.  If the largest tail
 *                  value equals the smallest, or if x_q = 0 with q = floor(M / 4 + 0.5) (1-based), then khat = +inf and
 *                  the raw weights stand.  Tied values have equal l, so which of them lands in the tail changes no
 *                  output beyond the summation order.
 *   Zhang-Stephens fit, as loo::gpdfit.  m = 30 + floor(sqrt(M)).
 *                  theta_j = 1 / x_M + (1 - sqrt(m / (j - 1/2))) / (3 x_q) for j = 1 .. m.
 *                  k_j = mean_i log1p(-theta_j x_i).
 *                  L_j = M (log(-theta_j / k_j) - k_j - 1).
 *                  w_j = 1 / sum_i exp(L_i - L_j).  An overflow to +inf is intended and gives weight 0.
 *                  theta^ = sum_j theta_j w_j, k = mean_i log1p(-theta^ x_i), sigma = -k / theta^.
 *                  khat = (k M + 5) / (M + 10).
 *   Smoothed tail. If khat is finite, the i-th tail sample (ascending, i = 1 .. M) gets
 *                  log(sigma expm1(-khat log1p(-p_i)) / khat + exp(c)) with p_i = (i - 1/2) / M.
 *   Truncate and normalise.  All log weights are truncated at 0.  Then lw_s -= logsumexp(lw).
 *   Per pixel.     elpd_loo_p = logsumexp_s(l_s + lw_s).  p_loo_p = lppd_p - elpd_loo_p, with lppd_p as in vamp_pred.h.
 *   Per group, summed in pixel order.  elpd_loo = sum_p elpd_loo_p.  elpd_loo_se = sqrt(P var_p) with P - 1 in the
 *                  denominator, and NaN for P < 2.  p_loo = sum_p p_loo_p.  n_high_k = #{p : khat_p > 0.7}.
 *   Edge rules.    n = 0: everything is NaN and it is not an error.  Any NaN or +-inf among a pixel's n values makes
 *                  that pixel's elpd_loo, p_loo and khat NaN.  lppd keeps vamp_pred.h's rule.  A NaN khat is not
 *                  counted in n_high_k.
 * Everything is fp64.
 *
 * Output, host arrays in group order; any pointer may be NULL:
 *   elpd_loo_pix, p_loo_pix, khat, lppd            sum of n_pix doubles
 *   elpd_loo, elpd_loo_se, p_loo                   G doubles
 *   n_high_k, n_used, n_bad                        G int32
 *   ll (vamp_loo_pointwise)                        G pointers; ll[g] is NULL or a host [S x n_pix[g]] matrix, sample-major
 *                                                  (ll[g][s * n_pix[g] + p]): the l_sp the call used, with the rows of
 *                                                  bad samples set to NaN
 *
 * Every function returns 0 on success and -1 on an error; vamp_loo_last_error() then says why.  Every
 * argument is checked before the first HIP call.  The caller's current HIP device is restored before return.
 */
#ifndef VAMP_LOO_H
#define VAMP_LOO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_LOO_ABI_VERSION 1
#define VAMP_LOO_MAX_SAMPLES 16384      /* as VAMP_PRED_MAX_SAMPLES: one time step serves the three libraries */
#define VAMP_LOO_MAX_COMPONENTS 32

int vamp_loo_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_loo_last_error(void);

/* PSIS-LOO of chains.  device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default
 * stream.  is_device: 0 = every base[g] is host memory (copied to one device staging buffer), 1 = device memory.
 * scratch_bytes: bound of the log-likelihood scratch of one pass (0 = 256 MiB); at least one column (8 S bytes) of
 * the largest group.  No result depends on it. */
int vamp_loo_pointwise(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                       const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                       const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                       const int32_t* n_keep, const int32_t* walkers, int64_t scratch_bytes, double* elpd_loo_pix,
                       double* p_loo_pix, double* khat, double* lppd, double* elpd_loo, double* elpd_loo_se, double* p_loo,
                       int32_t* n_high_k, int32_t* n_used, int32_t* n_bad, double* const* ll);

/* PSIS-LOO of log-likelihood matrices the caller already has.  ll[g]: [n_samples[g] x n_pix[g]], sample-major, every
 * one host memory (is_device = 0; copied to one device staging buffer) or device memory (1); 1 <= n_samples[g] <=
 * VAMP_LOO_MAX_SAMPLES.  skip: NULL, or G pointers; skip[g] is NULL or n_samples[g] bytes of HOST memory, 1 = leave the
 * sample out (it is counted in n_bad and its row is not read).  The other arguments and the outputs as above. */
int vamp_loo_from_loglik(int device, void* hip_stream, int n_groups, const double* const* ll, int is_device,
                         const int32_t* n_samples, const int32_t* n_pix, const uint8_t* const* skip, int64_t scratch_bytes,
                         double* elpd_loo_pix, double* p_loo_pix, double* khat, double* lppd, double* elpd_loo,
                         double* elpd_loo_se, double* p_loo, int32_t* n_high_k, int32_t* n_used, int32_t* n_bad);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_LOO_H */
