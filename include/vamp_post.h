/* vamp_post.h -- posterior summaries of ensemble chains on the GPU (libvamp_post.so).
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h) and libvamp_diag.so
 * (include/vamp_diag.h): it reads chains wherever they are -- host arrays, or the device chain
 * vamp_sampler_run_dev wrote -- and shares no state with a vamp_ctx.  Definitions: DESIGN.md "Posterior summaries".
 *
 * Input: G groups (one region's ensemble each).  Group g has
 *   x[g][n_pix[g]]   the abscissa (HOST memory, finite), in the units of the chain's centroids and widths
 *   n_comp[g] = K    lines, 1 <= K <= VAMP_POST_MAX_COMPONENTS
 *   mode[g]          0 = GAUSS3 (A, c, sigma) or 1 = VOIGT4 (A, c, L_fwhm, G_fwhm) per line: the layouts of
 *                    enum vamp_mode.  Mode 2 (NBZ3) is rejected.  q = 3 or 4 parameters per line.
 *   sample_sd[g]     1: the chain's last dimension is the free sd, which the model does not read.  D = q K + sample_sd.
 *   the chain, as vamp_diag_chains takes it: n_keep[g] = N kept samples of walkers[g] = W walkers; parameter d
 *                    of sample (t, w) is base[g][t * ld[g] + w * D + d], ld[g] >= W * D.  Sample index s = t * W + w,
 *                    S = N * W <= VAMP_POST_MAX_SAMPLES: a longer chain is an error, not truncated (subsample in
 *                    time by passing ld * step and ceil(N / step)).
 *   pixel_width[g]   the decrement sums are multiplied by it (finite)
 * and per call probs[n_probs], 1 <= n_probs <= VAMP_POST_MAX_PROBS, every p in [0, 1].
 *
 * Per sample: flux_p = exp(-sum_k tau_k(x_p)), EW = width * sum_p (1 - flux_p), EW_k = width * sum_p (1 - exp(-tau_k(x_p)))
 * (sums in pixel order).  A sample is BAD when one of its q K parameters is not finite, or sigma <= 0, or
 * G_fwhm <= 0, or L_fwhm < 0; bad samples are left out of every statistic and counted.  Over the n = S - n_bad others:
 * the mean, the population standard deviation about the mean, and numpy's default ("linear") quantiles of the
 * exact order statistics.  n = 0: every statistic is NaN; it is not an error.  A good sample's value may still be
 * NaN or infinite (an overflowing amplitude): a NaN among the n values of a column makes every statistic of that
 * column NaN, and an infinite value is treated as numpy treats it -- the mean is infinite, the standard deviation
 * NaN, and a quantile whose interpolation touches the infinite order statistic with weight 0 is NaN (inf - inf),
 * also at p = 0 and p = 1.
 *
 * Output, host arrays in group order; any pointer may be NULL:
 *   flux_mean, flux_sd      sum of n_pix doubles
 *   flux_q                  per group a [n_probs][n_pix] block, the groups' blocks one after the other
 *   ew_mean, ew_sd          G doubles;                     ew_q       [G][n_probs]
 *   comp_ew_mean, comp_ew_sd   sum of n_comp doubles;      comp_ew_q  [sum of n_comp][n_probs]
 *   n_used, n_bad           G int32
 *
 * Every function returns 0 on success and -1 on an error; vamp_post_last_error() then says why.  Every
 * argument is checked before the first HIP call.  The caller's current HIP device is restored before return.
 */
#ifndef VAMP_POST_H
#define VAMP_POST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_POST_ABI_VERSION 1
#define VAMP_POST_MAX_SAMPLES 16384      /* one column of doubles in 128 KiB of LDS */
#define VAMP_POST_MAX_COMPONENTS 32
#define VAMP_POST_MAX_PROBS 16

int vamp_post_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_post_last_error(void);

/* device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default stream.
 * is_device: 0 = every base[g] is host memory (copied to one device staging buffer), 1 = device memory.
 * scratch_bytes: bound of the flux scratch of one pass (0 = 256 MiB); at least one column (8 S bytes) of the
 * largest group. */
int vamp_post_summaries(int device, void* hip_stream, int n_groups, const double* const* x, const int32_t* n_pix,
                        const int32_t* n_comp, const int32_t* mode, const int32_t* sample_sd,
                        const double* const* base, int is_device, const int64_t* ld, const int32_t* n_keep,
                        const int32_t* walkers, const double* pixel_width, int n_probs, const double* probs,
                        int64_t scratch_bytes, double* flux_mean, double* flux_sd, double* flux_q, double* ew_mean,
                        double* ew_sd, double* ew_q, double* comp_ew_mean, double* comp_ew_sd, double* comp_ew_q,
                        int32_t* n_used, int32_t* n_bad);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_POST_H */
