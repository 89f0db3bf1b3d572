/* vamp_hmc.h -- Hamiltonian Monte Carlo chains per region on the GPU (libvamp_hmc.so): C independent chains per region,
 * each L leapfrog steps per move in the metric of a given factor, started at given points, with the exact log-posterior
 * and its analytic gradient.  The step loop is resident: one launch per call.
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h) and the other side libraries; it shares
 * no state with a vamp_ctx.  Definitions: below, and DESIGN.md section 17, "Preconditioned HMC".
 * Source: Duane, Kennedy, Pendleton & Roweth (1987), Phys. Lett. B 195, 216; Neal, "MCMC using Hamiltonian dynamics"
 * (2011); Salmon, Moraes, Dror & Shaw (SC'11) for Philox.
 *
 * Input: G groups (one region each).  Group g has
 *   x[g][n_pix[g]]       the abscissa (HOST memory, finite, strictly monotonic); P = n_pix[g] >= 1
 *   flux[g][n_pix[g]]    the data (HOST memory, finite)
 *   noise[g][n_pix[g]]   HOST memory, finite and > 0; NULL exactly when sample_sd[g] = 1
 *   n_comp[g] = K        lines, 1 <= K <= VAMP_HMC_MAX_COMPONENTS
 *   mode[g]              0 = GAUSS3 (A, c, sigma) or 1 = VOIGT4 (A, c, L_fwhm, G_fwhm) per line.  Mode 2 (NBZ3) is rejected.
 *   sample_sd[g]         1: the vector's last entry is the free sd, the noise of every pixel.  D = q K + sample_sd <= 65.
 *   bounds[g]            {c_lo, c_hi, sigma_max, fwhm_max} (HOST), or NULL (also bounds itself) to derive them from x as
 *                        vamp_evid.h does: c in [min x, max x], sigma_max = (max x - min x) / 2, fwhm_max = sigma_max
 *                        2 sqrt(2 ln 2).  A region of one pixel needs bounds.
 *   region_id[g]         >= 0, below 2^31: the group's identity in the draw keys
 *   n_chains[g] = C      >= 1 chains; chain_id0[g] >= 0.  Chain i of the group has identity c = chain_id0 + i, c < 2^26.
 *   start[g][C][D]       where the chains start; HOST memory, or DEVICE memory if start_is_device = 1
 *   chol[g][D][D]        the lower factor C of the inverse mass matrix M^-1 = C C^T, row-major (HOST).  Only the lower
 *                        triangle is read.
 *   eps[g] > 0           the step size;  jitter[g] in [0, 1) its relative jitter
 * Per call: n_leap = L (1 <= L <= VAMP_HMC_MAX_LEAP), n_steps >= 1, 0 <= n_burn < n_steps, thin >= 1, step0 >= 0 with
 * step0 + n_steps <= 2^31, and seed.  n_keep = the number of steps t in 0 .. n_steps - 1 with t >= n_burn and
 * (t - n_burn) mod thin = 0.  The draws of step t are keyed by T = step0 + t, so that a second call with step0 advanced
 * by the first call's n_steps, started at the first call's `last`, continues the run; n_burn and thin count from the
 * call's own t = 0.
 *
 * Target: ln p = ln pi + ln L exactly as vamp_evid.h and vamp_laplace.h define it -- priors A e^-A on amplitudes, uniform
 * centres and widths, sd ~ U(0, 1); the normalisation of ln L always included; a width of exactly 0 is outside.  Outside
 * the prior ln p = -inf and nothing is evaluated.  The gradient is vamp_fisher.h's grad with with_prior = 1:
 *   grad_d = sum_p J_pd r_p / sigma_p^2 + (1 / A_k - 1 on amplitude entries);   free sd: sum_p r_p^2 / sd^3 - P / sd
 * with J_pd = -f_p dtau_p / dtheta_d of that header.  It is the gradient of ln p at every interior point (the uniform
 * priors are flat; tests/test_hmc.py holds the two headers to each other by central differences); where they could
 * differ, ln p is the rule for the accept test and grad the rule for the trajectory.  Value and gradient come from one
 * pass over the pixels.  Sums over the pixels, in an order that depends on the group alone:
 *   chi^2     lane l of 64 adds (r_p / sigma_p)^2 over p = l, l + 64, ... ascending by fma from 0; the 64 sums are added by
 *             a butterfly over lane distances 32, 16, 8, 4, 2, 1
 *   grad_d    the terms (dtau_p / dtheta_d) (-f_p r_p / sigma_p^2) (sigma_p = 1 with the free sd, and the sum divided by
 *             sd^2) over p ascending, by fma from 0
 *
 * Draws for step T of chain c, keyed so that a chain gives the same bits alone or in any batch:
 *   momentum pairs j = 0 .. ceil(D / 2) - 1:
 *     (c0, c1, c2, c3) = philox4x32_10({T, c 64 + j, 6, region_id}, seed lo, seed hi)          (6 = STREAM_MOMENTUM)
 *     u1 = 1 - u53(c0, c1) in (0, 1],  u2 = u53(c2, c3),  u53(hi, lo) = ((hi << 32 | lo) >> 11) 2^-53
 *     rho = sqrt(-2 log u1),  z_2j = rho cos(2 pi u2),  z_2j+1 = rho sin(2 pi u2); the last z of an odd D is dropped
 *   (c0, c1, c2, c3) = philox4x32_10({T, c 64 + 63, 7, region_id}, seed lo, seed hi)            (7 = STREAM_HMC_ACCEPT)
 *     u = 1 - u53(c0, c1) in (0, 1] for the accept test;  u' = u53(c2, c3);  eps_t = eps (1 + jitter (2 u' - 1))
 * Stream ids 6 and 7 stand beside 0 - 5 of the other libraries.  If mom_in[g] (HOST) is given, its [n_steps][C][D] momenta
 * replace the z of every step; u and u' stay keyed.
 *
 * One step from the state (theta, ln p, g = grad at theta):
 *   p <- z
 *   H0 = ln p - kin(p) / 2,      kin(p) = sum_d p_d^2, the fma chain over d ascending from 0
 *   p_e <- fma(eps_t / 2, v_e, p_e),   v_e = (C^T g)_e: the fma chain of C_de g_d over d = e .. D - 1 ascending, from 0
 *   repeat L times:
 *       theta_d <- fma(eps_t, w_d, theta_d),   w_d = (C p)_d: the fma chain of C_de p_e over e = 0 .. d ascending, from 0
 *       evaluate (ln p, g) at theta
 *       if the point is outside the prior, bad by vamp_post.h's rule, or ln p is not finite: stop -- a wall
 *       p_e <- fma(h, v_e, p_e) with the new g;   h = eps_t, or eps_t / 2 after the last position update
 *   dH = (ln p' - kin(p') / 2) - H0
 *   accept iff log u < dH  (a NaN dH rejects): the state becomes (theta', ln p', g'); else it stays, g included
 * A wall rejects the step, counts in n_wall and has dH = NaN; the state is unchanged bit for bit.  A step costs exactly
 * L evaluations, or fewer at a wall.  A chain's bits do not depend on the rest of the call, on the other chains of its
 * group, on host or device arrays, or on the stream.
 *
 * status[g] (none is an error of the call):
 *   0  ok
 *   1  no factor: a diagonal entry of chol that is not finite or <= 0, a read entry (lower triangle) that is not finite,
 *      or an eps that is not finite or <= 0 or a jitter outside [0, 1).  Every output of the group is NaN, the counts 0
 *      and chain_status 1.
 * chain_status (per chain):
 *   0  ok
 *   2  the start is rejected by the target's own rule (outside the prior, bad, or ln p not finite).  That chain's
 *      outputs are NaN, its counts 0 and its acc 0.  The other chains run.
 *
 * Output; any pointer may be NULL, and so may an entry of a list of pointers:
 *   chain[g]    [n_keep][C][D]: the state after every kept step, in the layout vamp_diag.h reads (walkers = C);
 *               DEVICE memory if out_is_device = 1, else HOST
 *   last[g]     [C][D]: the state after the last step; DEVICE or HOST as chain
 *   lnp[g]      [n_keep][C] (HOST): ln p of the kept states
 *   n_accept, n_wall, chain_status      sum of C int32 (HOST), the groups one after the other
 *   dH_mean, dH_max                     sum of C doubles (HOST): mean and maximum of |dH| over the steps that met no wall,
 *                                       the mean summed in step order; NaN if every step met a wall
 *   status                              G int32 (HOST)
 * Traces (HOST), one entry per step t of the call:
 *   mom[g], prop[g], prop_mom[g]        [n_steps][C][D]: the momentum p the step started with, and the proposal's theta'
 *                                       and p' (at a wall: the rejected position and the momentum as it stood there)
 *   dH[g]                               [n_steps][C]
 *   acc[g]                              [n_steps][C] int32: 0 = rejected, 1 = accepted, 2 = wall
 * Limits: sum_g n_keep C D <= VAMP_HMC_MAX_CHAIN_DOUBLES, and sum_g n_steps C D within the same bound whenever a
 * trace or mom_in is given.
 *
 * Every function returns 0 on success and -1 on an error; vamp_hmc_last_error() then says why.  Every argument is
 * checked before the first HIP call.  The caller's current HIP device is restored before return.  Everything is fp64.
 */
#ifndef VAMP_HMC_H
#define VAMP_HMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_HMC_ABI_VERSION 1
#define VAMP_HMC_MAX_COMPONENTS 16
#define VAMP_HMC_MAX_DIM 65                               /* 4 * 16 + 1 */
#define VAMP_HMC_MAX_LEAP 64
#define VAMP_HMC_MAX_CHAIN_ID (1 << 26)
#define VAMP_HMC_MAX_CHAIN_DOUBLES (1LL << 28)            /* 2 GiB of kept states */

int vamp_hmc_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_hmc_last_error(void);

/* device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default stream. */
int vamp_hmc_chains(int device, void* hip_stream, int n_groups, const double* const* x, const double* const* flux,
                    const double* const* noise, const int32_t* n_pix, const int32_t* n_comp, const int32_t* mode,
                    const int32_t* sample_sd, const double* const* bounds, const int32_t* region_id, const int32_t* n_chains,
                    const int32_t* chain_id0, const double* const* start, int start_is_device, const double* const* chol,
                    const double* eps, const double* jitter, int n_leap, int n_steps, int n_burn, int thin, int64_t step0,
                    uint64_t seed, const double* const* mom_in, double* const* chain, double* const* last, int out_is_device,
                    double* const* lnp, int32_t* n_accept, int32_t* n_wall, double* dH_mean, double* dH_max,
                    int32_t* chain_status, int32_t* status, double* const* mom, double* const* prop, double* const* prop_mom,
                    double* const* dH, int32_t* const* acc);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_HMC_H */
