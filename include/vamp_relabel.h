/* vamp_relabel.h -- undo label switching: the optimal relabelling of the lines of ensemble chains on the GPU
 * (libvamp_relabel.so).
 *
 * Plain C99.  A library of its own, beside libvamp_hip.so (include/vamp_hip.h), libvamp_diag.so (include/vamp_diag.h),
 * libvamp_post.so (include/vamp_post.h), libvamp_evid.so (include/vamp_evid.h), libvamp_pred.so (include/vamp_pred.h)
 * and libvamp_loo.so (include/vamp_loo.h): it reads chains wherever they are -- host arrays, or the device chain
 * vamp_sampler_run_dev wrote -- and shares no state with a vamp_ctx.  It moves parameters and never evaluates a line.
 * Definitions: below, and word for word in DESIGN.md "Relabelling: undoing label switching".
 * Source: Stephens (2000), J. R. Statist. Soc. B 62, 795; Celeux (1998), COMPSTAT 98, 227; Cron & West (2011),
 * Statistical Applications in Genetics and Molecular Biology 10, 1 (the k-means form: assign, move the reference,
 * repeat).  The assignment is the shortest-augmenting-path form of the Hungarian method (Jonker & Volgenant 1987).
 *
 * The K lines of a region are exchangeable, so the posterior has K! copies of every mode and a walker may sit in any
 * of them.  For every sample the library finds the permutation of its lines that lies closest to a reference
 * labelling, then moves the reference to the means of the relabelled samples and repeats until nothing changes.
 *
 * Input: G groups in the chain layout of vamp_pred.h.  Per group n_comp = K with 1 <= K <= VAMP_RELABEL_MAX_COMPONENTS;
 * mode 0 = GAUSS3 (q = 3 parameters per line), 1 = VOIGT4 (q = 4), mode 2 is rejected; sample_sd, so D = q K + sd;
 * base, is_device, ld, n_keep, walkers as there, with no limit on the samples beyond S = n_keep * walkers < 2^31: a
 * relabelled chain must cover the whole chain.  ref[g]: K x q host doubles, finite, the reference labelling (line j's
 * parameters at ref[g][q j ..]).  scale: NULL, or G pointers; scale[g] is NULL or q host doubles, finite and > 0.
 * max_iter >= 1.
 *
 * Definitions.
 *
 * - *Line vector.* `v_si[d] = θ_s[q i + d]`, the d-th parameter of line i of sample s = t·W + w.
 * - *Bad sample.* Any of its qK line parameters is not finite. The sd is not looked at and no width is tested: relabelling moves parameters, it does not evaluate them. Bad samples:
 *   - keep the identity permutation;
 *   - get cost NaN;
 *   - are copied unchanged;
 *   - are counted in `n_bad`;
 *   - enter no statistic and no other count.
 * - *Scale.* If `scale[g]` is NULL, `scale[d]` is the standard deviation (denominator n − 1) of parameter d pooled over all K lines and all good samples. Where that is 0 or not finite, or there are fewer than two values, it is 1. The scale is fixed for the whole call.
 * - *Cost.* `C_s(i, j) = Σ_d ((v_si[d] − ref_j[d]) / scale[d])²`, summed in d order.
 * - *Assignment.* `π_s` is a permutation of 0 .. K−1 that minimises `Σ_j C_s(π(j), j)`: label j is given to the sample's line π(j).
 *   - Where several permutations attain the minimum, any of them may be returned.
 *   - The result for a sample depends on that sample, `ref` and `scale` only. It does not depend on its neighbours in a lane group, the batch, the packing or the stream.
 * - *Relabelled sample.* Line j ← `v_{s,π(j)}`. The sd and any padding between `W·D` and `ld` are untouched.
 * - *Rounds.*
 *   - Round 1 assigns against `ref`.
 *   - After round r, `ref_{r+1}[j][d]` is the mean of the relabelled `v_sj[d]` over the good samples, summed in a fixed order.
 *   - `n_changed_r` is the number of good samples whose π differs from the previous round's. Round 0 is the identity.
 *   - A group's `n_iter` is the first r > 1 with `n_changed_r` = 0. If there is none, it is `max_iter`.
 *   - All outputs describe round `n_iter`.
 *   - The reductions have a fixed order. A group that has stopped changing therefore reproduces its reference bit for bit, so running it further changes nothing. The host loop may run all groups until all have stopped, or stop at `max_iter`.
 * - *Per label.*
 *   - `label_mean[j][d]` and `label_sd[j][d]` (denominator n − 1) are taken over the good samples of the last round.
 *   - n = 0 gives NaN for both.
 *   - n = 1 gives sd NaN.
 * - *Per group.*
 *   - `n_switched` is the number of good samples with π ≠ identity.
 *   - `n_changed` is the last round's count. It is 0 exactly when the group converged; with `max_iter` = 1 it equals `n_switched`.
 *   - Also returned: `n_iter`, `n_used`, `n_bad`.
 * - Everything is fp64.
 *
 * Two notes on the edges.  A good sample whose cost matrix has an entry that is not finite (an overflow of the squares)
 * keeps the identity permutation and gets cost NaN like a bad one, but stays a good sample: it is counted in n_used and
 * enters the means.  So does a sample whose entries are finite but so large (|C| K near DBL_MAX) that a potential or the
 * total overflows inside the solver: the solver's loops end all the same, and a result that is not a permutation with a
 * finite total is discarded.  A caller reads convergence as n_changed = 0 AND n_iter > 1: one round alone (max_iter = 1) has
 * compared its permutations with the identity only, which is n_switched.
 *
 * Output; any pointer may be NULL:
 *   out, out_ld, out_is_device     out: NULL, or G pointers; out[g] is NULL or the relabelled chain of group g, rows
 *                                  out_ld[g] doubles apart, host (out_is_device = 0) or device (1) memory.  out[g] may
 *                                  equal base[g] with out_ld[g] = ld[g] and out_is_device = is_device, which relabels in
 *                                  place; otherwise it must not overlap base[g].  Out of place the whole sample is
 *                                  written, its sd included; the padding of out is not written.
 *   perm                           NULL, or G pointers; perm[g] is NULL or [S][K] uint8 on the host: perm[g][s K + j] = π_s(j)
 *   cost                           NULL, or G pointers; cost[g] is NULL or [S] doubles on the host: the attained total
 *   label_mean, label_sd           sum of K q doubles, group after group, [j][d] in a group
 *   scale_used                     sum of q doubles
 *   n_iter, n_changed, n_switched, n_used, n_bad       G int32
 *
 * Every function returns 0 on success and -1 on an error; vamp_relabel_last_error() then says why.  Every argument is
 * checked before the first HIP call.  The caller's current HIP device is restored before return.
 */
#ifndef VAMP_RELABEL_H
#define VAMP_RELABEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_RELABEL_ABI_VERSION 1
#define VAMP_RELABEL_MAX_COMPONENTS 32

int vamp_relabel_version(void);

/* message of the last failed call of this thread ("" if none) */
const char* vamp_relabel_last_error(void);

/* Relabels chains.  device: HIP device to run on; hip_stream: a hipStream_t of that device, or NULL for the default
 * stream.  is_device: 0 = every base[g] is host memory (copied to one device staging buffer), 1 = device memory. */
int vamp_relabel_chains(int device, void* hip_stream, int n_groups, const int32_t* n_comp, const int32_t* mode,
                        const int32_t* sample_sd, const double* const* base, int is_device, const int64_t* ld,
                        const int32_t* n_keep, const int32_t* walkers, const double* const* ref, const double* const* scale,
                        int max_iter, double* const* out, const int64_t* out_ld, int out_is_device, uint8_t* const* perm,
                        double* const* cost, double* label_mean, double* label_sd, double* scale_used, int32_t* n_iter,
                        int32_t* n_changed, int32_t* n_switched, int32_t* n_used, int32_t* n_bad);

/* A test hook: solves n arbitrary K x K cost matrices with the device function the chain kernel uses.  cost: host
 * [n][K][K], cost[(m K + i) K + j] = C_m(i, j); perm: NULL or host [n][K], perm[m K + j] = π_m(j); total: NULL or host
 * [n], the attained Σ_j C_m(π(j), j).  A matrix with an entry that is not finite gives the identity permutation and
 * total NaN; so does one whose finite entries overflow inside the solver (|C| K near DBL_MAX).  1 <= K <= VAMP_RELABEL_MAX_COMPONENTS, 1 <= n, n K K < 2^31. */
int vamp_relabel_assign(int device, int K, int n, const double* cost, uint8_t* perm, double* total);

#ifdef __cplusplus
}
#endif

#endif /* VAMP_RELABEL_H */
