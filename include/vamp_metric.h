/* vamp_metric.h -- a positive-definite metric from any symmetric matrix, per region, on the GPU (libvamp_metric.so): the
 * eigen-decomposition of the matrix in units of the parameters' prior standard deviations, its eigenvalues clamped to
 * [lam_lo, lam_hi], and from them a covariance, a precision, ln det and the Cholesky factor that vamp_hmc.h and
 * vamp_laplace.h take -- with the count of directions that had to be repaired.
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h) and the other side libraries; it shares
 * no state with a vamp_ctx and never sees parameters or data.  Definitions: below, and DESIGN.md section 18,
 * "Regularised metric".  Source: Jacobi (1846); Brent & Luk (1985) for the round-robin ordering of disjoint pairs;
 * Golub & Van Loan, "Matrix Computations", section 8.5 for the rotation.
 *
 * Input: G groups.  Group g has
 *   dim[g] = D           1 <= D <= VAMP_METRIC_MAX_DIM
 *   n_mat[g] = M         >= 1 symmetric matrices
 *   mat[g]               the M matrices [D][D] one after the other, row-major, ld[g] >= D doubles between two rows (and
 *                        between the last row of a matrix and the first of the next): entry (i, j) of matrix m is
 *                        mat[g][(m D + i) ld + j].  Only the lower triangle (j <= i) is read.  HOST memory, or DEVICE
 *                        memory if is_device = 1.  From host memory the (M D - 1) ld + D doubles from mat[g] on are copied.
 *   scale[g][D]          s_d: the prior standard deviations (HOST), finite and > 0
 *   kind[g]              0 = the matrices are informations H (inverse covariances), 1 = covariances S
 *   lam_lo[g] > 0, lam_hi[g] >= lam_lo[g] (+inf is allowed)
 * Per call: n_sweeps in 1 .. VAMP_METRIC_MAX_SWEEPS.  Limit: sum_g M D^2 <= VAMP_METRIC_MAX_MATRIX_DOUBLES (and the doubles
 * copied from host memory within the same bound).
 *
 * Per matrix, everything in fp64:
 * 1. Scaling, for j <= i, mirrored to (j, i):
 *      kind 0:  B_ij = (s_i H_ij) s_j            kind 1:  B_ij = S_ij / (s_i s_j)
 *    In these units an eigenvalue of the information below 1 is a direction the data constrain less than the prior.
 *    ||B||_F = sqrt(sum_i r_i), r_i = the fma chain of B_ij^2 over j = 0 .. D - 1 ascending from 0, the r_i added over
 *    i ascending from 0.  tol = 2^-52 ||B||_F.  A read entry or a B_ij that is not finite, or a norm that is not, gives
 *    status 2.
 * 2. Eigen-decomposition by cyclic two-sided Jacobi.  n = D rounded up to even; a pad row and column are zero (and
 *    never rotate).  A = B, V = I.  A sweep is the rounds r = 0 .. n - 2.  Round r pairs the slots idx[k] and idx[n-1-k],
 *    k = 0 .. n/2 - 1, where idx[0] = 0 and idx[k] = 1 + (r + k - 1) mod (n - 1): the pairs of a round are disjoint, and
 *    a sweep meets every pair once.  With p < q the two slots of a pair and a_pq read from the lower triangle (row q),
 *    the pair rotates iff |a_pq| > tol:
 *      tau = (a_qq - a_pp) / (2 a_pq),  t = sign(tau) / (|tau| + sqrt(fma(tau, tau, 1))),  sign(0) = +1
 *      c = 1 / sqrt(fma(t, t, 1)),  s = t c
 *    All (c, s) of a round are taken from the matrix as it stood before the round.  Then, for every rotating pair,
 *      rows:     (a_pj, a_qj) <- (fma(c, a_pj, -(s a_qj)), fma(s, a_pj, c a_qj))     for all j
 *      columns:  (a_ip, a_iq) <- (fma(c, a_ip, -(s a_iq)), fma(s, a_ip, c a_iq))     for all i, after all rows
 *      V:        (v_ip, v_iq) likewise
 *      a_pq = a_qp = 0 exactly.
 *    The sweep loop runs at most n_sweeps times and ends after a sweep in which no pair rotated; sweeps_used counts the
 *    sweeps run, that last one included (the identity: 1).  Then off = max |a_pq| over p != q; off > tol gives status 3.
 * 3. eig = the diagonal a_dd, d < D, sorted ascending, ties by slot; column i of vec [D][D] (row-major) is the column of
 *    V of the slot of eig_i.
 *      kind 0: lam_i = eig_i          kind 1: lam_i = 1 / eig_i if eig_i > 0, else +inf
 *      lam~_i = min(max(lam_i, lam_lo), lam_hi);   n_low = #{lam_i < lam_lo},  n_high = #{lam_i > lam_hi}
 * 4. For b <= a, mirrored:
 *      cov_ab  = (s_a C_ab) s_b,   C_ab = the chain c <- fma(vec_ai (1 / lam~_i), vec_bi, c) over i ascending from 0
 *      prec_ab = (P_ab / s_a) / s_b,   P_ab = the chain with lam~_i in place of 1 / lam~_i
 *      logdet  = (sum_i ln lam~_i, i ascending) - 2 (sum_d ln s_d, d ascending): ln det of the regularised information
 *    (lam_hi = +inf and an infinite lam_i leave prec without a finite value.)
 * 5. chol = the lower Cholesky factor of cov: with q_a = sqrt(cov_aa), L L^T = (cov_ab / (q_a q_b)) by vamp_fisher.h's rule
 *    -- a pivot must be above D 2^-52, and every cov_aa positive and finite -- and chol_ab = q_a L_ab, the upper triangle 0.
 *    A failed pivot gives status 1.
 *
 * status, per matrix (none is an error of the call):
 *   0  ok
 *   1  cov does not factor: chol is NaN, everything else is returned
 *   2  a read entry is not finite: every output of the matrix is NaN, its counts and sweeps_used 0
 *   3  not converged in n_sweeps: eig, vec, n_low, n_high, sweeps_used and off are returned; cov, prec, chol, logdet NaN
 *
 * Output, the matrices of group 0 first, each group's one after the other; any pointer may be NULL:
 *   eig                       sum of M D doubles (HOST)
 *   vec, prec                 sum of M D^2 doubles (HOST)
 *   cov, chol                 sum of M D^2 doubles: HOST, or DEVICE memory if out_is_device = 1
 *   logdet, off               sum of M doubles (HOST)
 *   n_low, n_high, sweeps_used, status      sum of M int32 (HOST)
 * A matrix's results depend on that matrix, its scales, kind, clamps and n_sweeps alone: they are the same bits alone, in
 * any batch, in any order, from host or device input, and on any stream.
 *
 * vamp_metric_plan says how a call whose largest D is max_dim is laid out: the matrices that share a workgroup (one
 * 64-lane wavefront each) and the dynamic LDS of that workgroup in bytes.
 *
 * Every function returns 0 on success and -1 on an error; vamp_metric_last_error() then says why.  Every argument is
 * checked before the first HIP call.  The caller's current HIP device is restored before return.
 */
#ifndef VAMP_METRIC_H
#define VAMP_METRIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_METRIC_ABI_VERSION 1
#define VAMP_METRIC_MAX_DIM 65                            /* 4 * 16 + 1 */
#define VAMP_METRIC_MAX_SWEEPS 32
#define VAMP_METRIC_MAX_MATRIX_DOUBLES (1LL << 27)        /* 1 GiB for each of vec, cov, prec and chol */

int vamp_metric_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_metric_last_error(void);

int vamp_metric_plan(int max_dim, int32_t* mats_per_workgroup, int64_t* lds_bytes);

/* device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default stream. */
int vamp_metric_factor(int device, void* hip_stream, int n_groups, const double* const* mat, int is_device, const int64_t* ld,
                       const int32_t* dim, const int32_t* n_mat, const double* const* scale, const int32_t* kind,
                       const double* lam_lo, const double* lam_hi, int n_sweeps, int out_is_device, double* eig, double* vec,
                       double* cov, double* prec, double* chol, double* logdet, int32_t* n_low, int32_t* n_high,
                       int32_t* sweeps_used, double* off, int32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_METRIC_H */
