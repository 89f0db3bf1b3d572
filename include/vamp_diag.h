/* vamp_diag.h -- convergence diagnostics of ensemble chains on the GPU (libvamp_diag.so).
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h): it reads chains
 * wherever they are -- host arrays, or the device chain vamp_sampler_run_dev wrote -- and shares no
 * state with a vamp_ctx.  Definitions: DESIGN.md "Chain diagnostics".
 *
 * Input: G groups (one ensemble each).  Group g has n_keep[g] = N kept samples of walkers[g] = W
 * walkers in ndim[g] = D parameters; sample (t, w, d) is base[g][t * ld[g] + w * D + d], ld[g] >= W * D.
 *   - a [N, W, D] array:                   base = the array, ld = W * D
 *   - region r of a vamp_sampler_run_dev chain [n_keep, total_theta]:
 *                                           base = chain + W * (sum of the ndims of regions < r), ld = total_theta
 *
 * Output, per (group, parameter), in group order (sum of ndim entries, host arrays):
 *   tau      integrated autocorrelation time, in kept samples (+inf: a walker's series is constant)
 *   n_eff    N * W / tau (NaN when tau <= 0)
 *   r_hat    split-R-hat (BDA3, not rank-normalised); NaN under the rule for values that are not finite, below
 *   window   the window M the sum of tau stops at (-1 when tau is +inf or NaN)
 *   reliable 1 when a window was found, tau > 0 and N >= 50 max(tau, 1): never for N < 50.  (tau_{N-1} = 0
 *            identically -- the centred series' autocovariances sum to zero -- so on a very short chain the window
 *            can land where tau_m has collapsed to about 0 or below; such a tau is reported but never trusted.)
 * A group with N < 4 gets NaN everywhere (window -1, reliable 0); it is not an error.
 * Values that are not finite: a NaN or +-inf anywhere in the series of any walker of a (group, parameter) gives
 * tau = n_eff = r_hat = NaN, window = -1 and reliable = 0 for that parameter.  This comes before "a walker's series
 * is constant" (a series that is constant but for a NaN is not finite, not stuck).  The other parameters of the
 * group are not affected.
 *
 * Every function returns 0 on success and -1 on an error; vamp_diag_last_error() then says why.
 * The caller's current HIP device is restored before return.
 */
#ifndef VAMP_DIAG_H
#define VAMP_DIAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_DIAG_ABI_VERSION 1
#define VAMP_DIAG_MAX_SAMPLES 8192   /* the direct lag sum is O(N^2): longer chains are rejected */

int vamp_diag_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_diag_last_error(void);

/* device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default stream.
 * is_device: 0 = every base[g] is host memory (copied to one device staging buffer), 1 = device memory.
 * c: the window factor (emcee's c, 5 by default in the Python API); must be > 0. */
int vamp_diag_chains(int device, void* hip_stream, int n_groups, const double* const* base, int is_device,
                     const int64_t* ld, const int32_t* n_keep, const int32_t* walkers, const int32_t* ndim,
                     double c, double* tau, double* n_eff, double* r_hat, int32_t* window, uint8_t* reliable);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_DIAG_H */
