/* vamp_fisher.h -- gradient of the log-posterior, Gauss-Newton information matrix and its inverse at given parameter
 * vectors, from the analytic Jacobian of the model flux, on the GPU (libvamp_fisher.so).
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h) and the other side libraries: it reads
 * parameter vectors wherever they are -- host arrays, or device memory such as a context's MAP -- and shares no state
 * with a vamp_ctx.  Definitions: DESIGN.md section 15, "Fisher-matrix errors at a point".
 *
 * Input: G groups (one region each).  Group g has
 *   x[g][n_pix[g]]       the abscissa (HOST memory, finite), in the units of the centroids and widths; P = n_pix[g] >= 1
 *   flux[g][n_pix[g]]    the data y_p (HOST memory, finite)
 *   noise[g][n_pix[g]]   HOST memory, finite and > 0; NULL exactly when sample_sd[g] = 1
 *   n_comp[g] = K        lines, 1 <= K <= VAMP_FISHER_MAX_COMPONENTS
 *   mode[g]              0 = GAUSS3 (A, c, sigma) or 1 = VOIGT4 (A, c, L_fwhm, G_fwhm) per line.  Mode 2 (NBZ3) is rejected.
 *   sample_sd[g]         1: the vector's last entry is the free sd, the noise of every pixel.  D = q K + sample_sd <= 65.
 *   the points           n_points[g] >= 1 vectors theta of D doubles; entry d of point i is base[g][i * ld[g] + d],
 *                        ld[g] >= D (ld[g] >= 0 when n_points[g] = 1)
 * with sum_g n_points[g] D_g^2 <= VAMP_FISHER_MAX_MATRIX_DOUBLES and, when jac is asked for, sum_g n_points[g] P_g D_g
 * within the same bound.
 *
 * Per point, with f_p = exp(-sum_k tau_k(x_p)), r_p = y_p - f_p and sigma_p = noise_p, or the point's sd:
 *   Voigt line, s = 2 sqrt(ln 2) / G, u = (x - c) s, y = L sqrt(ln 2) / G, w(u + i y) = K + i M:
 *     tau_k = A y sqrt(pi) K;   K_u = -2 (u K - y M),  K_y = 2 (u M + y K) - 2 / sqrt(pi)
 *     dtau/dA = y sqrt(pi) K                     dtau/dc = -A y sqrt(pi) s K_u
 *     dtau/dL = A sqrt(pi) (sqrt(ln 2) / G) (K + y K_y)
 *     dtau/dG = -(A sqrt(pi) y / G) (K + u K_u + y K_y)
 *   Gaussian line, u = (x - c) / sigma_k, e = exp(-u^2 / 2):
 *     tau_k = A e;   dtau/dA = e,   dtau/dc = A e u / sigma_k,   dtau/dsigma_k = A e u^2 / sigma_k
 *   J_pd   = df_p / dtheta_d = -f_p dtau_p / dtheta_d               (0 in the column of the free sd)
 *   chi2   = sum_p (r_p / sigma_p)^2
 *   grad_d = sum_p J_pd r_p / sigma_p^2 + (1 / A_k - 1 on amplitude entries);   free sd: sum_p r_p^2 / sd^3 - P / sd
 *   info   = sum_p J_p J_p^T / sigma_p^2 + diag(1 / A_k^2 on amplitude entries);   free sd: info_sd,sd = 2 P / sd^2 and
 *            zero cross terms (the expected information).  with_prior = 0 leaves out the two terms of the amplitudes'
 *            x e^-x prior (the uniform priors are flat).
 *   cov    = info^-1,   sigma_d = sqrt(cov_dd),   logdet = ln det info
 * Every sum runs in pixel order, so a point's results do not depend on what else is in the call: bit for bit.
 *
 * status of a point (neither is an error of the call):
 *   0  ok
 *   1  info is not positive definite: a zero diagonal entry, or a pivot of the Cholesky factorisation of the scaled
 *      matrix C_ij = info_ij / sqrt(info_ii info_jj) that is not above D 2^-52.  cov, sigma and logdet are NaN; grad,
 *      info, chi2 and jac are returned.
 *   2  a bad point: a line parameter that is not finite, sigma_k <= 0, G_fwhm <= 0 or L_fwhm < 0 (the rule of
 *      vamp_post.h), or a free sd that is not finite or <= 0.  Every output of the point is NaN.
 *
 * Output, HOST arrays, groups one after the other and a group's points in order; any pointer may be NULL:
 *   grad, sigma            sum of n_points D doubles
 *   info, cov              sum of n_points D^2 doubles: full symmetric [D][D], row-major
 *   logdet, chi2           sum of n_points doubles;   status: as many int32
 *   jac                    sum of n_points P D doubles: [P][D] per point
 *
 * Every function returns 0 on success and -1 on an error; vamp_fisher_last_error() then says why.  Every argument is
 * checked before the first HIP call.  The caller's current HIP device is restored before return.  Everything is fp64.
 */
#ifndef VAMP_FISHER_H
#define VAMP_FISHER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_FISHER_ABI_VERSION 1
#define VAMP_FISHER_MAX_COMPONENTS 16
#define VAMP_FISHER_MAX_DIM 65                            /* 4 * 16 + 1 */
#define VAMP_FISHER_MAX_MATRIX_DOUBLES (1LL << 26)        /* 512 MiB for each of info and cov (and of jac) */

int vamp_fisher_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_fisher_last_error(void);

/* device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default stream.
 * is_device: 0 = every base[g] is host memory (copied to one device staging buffer), 1 = device memory. */
int vamp_fisher_points(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                       const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                       const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                       const int32_t* n_points, int with_prior, double* grad, double* info, double* cov, double* sigma,
                       double* logdet, double* chi2, int32_t* status, double* jac);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_FISHER_H */
