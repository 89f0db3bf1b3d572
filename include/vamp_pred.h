/* vamp_pred.h -- pointwise log predictive density and WAIC of ensemble chains on the GPU (libvamp_pred.so).
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h), libvamp_diag.so (include/vamp_diag.h),
 * libvamp_post.so (include/vamp_post.h) and libvamp_evid.so (include/vamp_evid.h): it reads chains wherever they are
 * -- host arrays, or the device chain vamp_sampler_run_dev wrote -- and shares no state with a vamp_ctx.
 * Definitions: DESIGN.md "Pointwise predictive density and WAIC".
 *
 * Input: G groups (one region's ensemble each).  Group g has what vamp_post_summaries takes for it
 *   x[g][n_pix[g]]   the abscissa (HOST memory, finite), in the units of the chain's centroids and widths
 *   n_comp[g] = K    lines, 1 <= K <= VAMP_PRED_MAX_COMPONENTS
 *   mode[g]          0 = GAUSS3 (A, c, sigma) or 1 = VOIGT4 (A, c, L_fwhm, G_fwhm) per line.  Mode 2 (NBZ3) is rejected.
 *   sample_sd[g]     1: the chain's last dimension is the free sd, the noise of every pixel.  D = q K + sample_sd.
 *   the chain        n_keep[g] = N kept samples of walkers[g] = W walkers; parameter d of sample (t, w) is
 *                    base[g][t * ld[g] + w * D + d], ld[g] >= W * D.  Sample index s = t * W + w, S = N * W <=
 *                    VAMP_PRED_MAX_SAMPLES: a longer chain is an error, not truncated (subsample in time by passing
 *                    ld * step and ceil(N / step)).
 * and the data
 *   flux[g][n_pix[g]]    HOST memory, finite
 *   noise[g][n_pix[g]]   HOST memory, finite and > 0; NULL exactly when sample_sd[g] = 1
 *
 * A sample is BAD under vamp_post.h's rule (a parameter of the q K that is not finite, sigma <= 0, G_fwhm <= 0,
 * L_fwhm < 0) and, when sample_sd is set, when its sd is not finite or <= 0.  Bad samples are left out and counted.
 * Over the n = S - n_bad others, for pixel p, with f_sp the model flux exp(-sum_k tau_k(x_p)) of sample s:
 *   l_sp     = -1/2 ((y_p - f_sp) / sigma_sp)^2 - ln sigma_sp - 1/2 ln 2 pi     sigma_sp = noise_p, or sd_s
 *   lppd_p   = m_p + ln((1/n) sum_s exp(l_sp - m_p)),  m_p = max_s l_sp
 *   llmean_p = (1/n) sum_s l_sp
 *   pwaic_p  = sum_s (l_sp - llmean_p)^2 / (n - 1)                               (n < 2: NaN)
 *   elpd_p   = lppd_p - pwaic_p
 * and per group, summed in pixel order over the per-pixel values:
 *   elpd_waic = sum_p elpd_p, p_waic = sum_p pwaic_p, lnl_mean = sum_p llmean_p,
 *   elpd_se = sqrt(P var_p(elpd_p)) with P - 1 in the variance's denominator (P < 2: NaN),
 *   n_high = #{p : pwaic_p > 0.4}.
 * n = 0: every statistic is NaN; it is not an error.  A NaN l among a pixel's n values makes the pixel's three
 * statistics NaN.  l = -inf is treated as numpy treats it: lppd stays finite while another sample is finite, the mean
 * is -inf and the variance NaN.  Everything is fp64.
 *
 * Output, host arrays in group order; any pointer may be NULL:
 *   lppd, ll_mean, p_waic_pix                      sum of n_pix doubles
 *   elpd_waic, elpd_se, p_waic, lnl_mean           G doubles
 *   n_high, n_used, n_bad                          G int32
 *
 * Every function returns 0 on success and -1 on an error; vamp_pred_last_error() then says why.  Every
 * argument is checked before the first HIP call.  The caller's current HIP device is restored before return.
 */
#ifndef VAMP_PRED_H
#define VAMP_PRED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_PRED_ABI_VERSION 1
#define VAMP_PRED_MAX_SAMPLES 16384      /* as VAMP_POST_MAX_SAMPLES: one time step serves both libraries */
#define VAMP_PRED_MAX_COMPONENTS 32

int vamp_pred_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_pred_last_error(void);

/* device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default stream.
 * is_device: 0 = every base[g] is host memory (copied to one device staging buffer), 1 = device memory.
 * scratch_bytes: bound of the log-likelihood scratch of one pass (0 = 256 MiB); at least one column (8 S bytes) of
 * the largest group.  No result depends on it. */
int vamp_pred_pointwise(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                        const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                        const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                        const int32_t* n_keep, const int32_t* walkers, int64_t scratch_bytes, double* lppd,
                        double* ll_mean, double* p_waic_pix, double* elpd_waic, double* elpd_se, double* p_waic,
                        double* lnl_mean, int32_t* n_high, int32_t* n_used, int32_t* n_bad);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_PRED_H */
