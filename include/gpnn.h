/* gpnn.h — nearest-neighbour GP scoring of the resident candidates for 10^4 .. 10^6 observations, exported by libgpbo.so next to the
 * C ABI of gpbo.h.
 *
 * A header of its own for the reason gpls.h is: the library's gpbo_ exports are exactly what gpbo.h declares, and each of its
 * functions is classified by a closed table of the order-of-calls contract.  The call is declared here under the prefix gpnn_.
 * gpbo.h supplies gpbo_ctx, the status codes, the kernel and acquisition kinds and the limits; GPBO_ABI_VERSION does not change,
 * because nothing in gpbo.h changes meaning.  Valid C99 on its own.  The function is a reader in the order-of-calls sense. */
#ifndef GPNN_H
#define GPNN_H

#include "gpbo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPNN_MAX_N         (1 << 20)
#define GPNN_MAX_NEIGHBORS 64          /* k in {16, 32, 64} */

/* The nearest-neighbour GP (Vecchia 1988; Emery 2009; Datta, Banerjee, Finley & Gelfand 2016; Gramacy & Apley's laGP), also called
 * local kriging: at FIXED hyper-parameters a candidate's posterior is that of the exact GP conditioned on its k nearest observations
 * only.  Every other device path of this library is an exact GP — an O(N^3) fit, N^2 per candidate — and ends at N = 65536; this
 * one costs O(N d) per candidate for the search plus O(k^3) for a small solve, needs no fit and no N x N matrix, and takes N up to
 * GPNN_MAX_N.  No model slot is read or written: the model is the call's own arguments.
 *
 * Inputs.  X (N, d) and y_norm (N,): host, the observations in parameter space and their NORMALISED targets; copied into workspace
 * the context owns (grown on demand and kept), the rows divided by the length scales once, on the device (true division, as the
 * fit's).  The candidates are the context's resident ones (gpbo_set_candidates, gpbo_generate_candidates*), M of them, divided by
 * the same length scales into the call's workspace.  kernel, length_scale / n_ls, amplitude = c, alpha: as in gpbo_fit_scaled.
 * white is taken RELATIVE TO THE AMPLITUDE: the matrix below has c white + alpha on its diagonal, so a slot fitted by
 * gpbo_fit_scaled(amplitude, white, alpha) is this call's (amplitude, white / amplitude, alpha); a unit model is amplitude = 1,
 * white = 0.  acq: GPBO_ACQ_UCB, GPBO_ACQ_EI, GPBO_ACQ_POI or GPBO_ACQ_LOG_EI with kappa_or_xi and y_max as in gpbo_acq_argbest.
 *
 * Neighbours.  With xs = x / length_scale and Xs_i = X_i / length_scale, d2_i = sum_t (xs_t - Xs_i,t)^2 in fp64, one fma per t, t
 * ascending from 0.  The neighbours of x are the k rows of smallest (d2_i, i) in lexicographic order — a tie in d2 goes to the lower
 * row index —, listed in that order: n_0 the nearest.  k is 16, 32 or 64 and N >= k; with N == k every row is a neighbour and the
 * result is the exact GP's.
 *
 * Per candidate, over its neighbours in that order (k(.) the unit kernel of `kernel` at the scaled squared distance, gpbo.h):
 *   A      = c K_nn + (c white + alpha) I        K_nn[a][b] = k(d2(X_na, X_nb)); the diagonal is c + (c white + alpha) exactly,
 *                                                rounded once on the host
 *   L      = chol(A)                             lower, column by column, right-looking: l_jj = sqrt(a_jj), l_ij = a_ij / l_jj,
 *                                                a_ib = fma(-l_ij, l_bj, a_ib) for j < b <= i
 *   v = L^-1 k*,  u = L^-1 y_nn                  k*_a = c k(d2(x, X_na)); forward substitution inside the same column sweep
 *   mu     = y_mean + y_std (v . u)              both sums by a butterfly over the k lanes (xor 1, 2, 4, ...)
 *   sd     = y_std sqrt(max(c - |v|^2, 0))       the latent function's deviation
 *   ys     = -acq(mu, sd)                        csrc/acq_formulas.h's functions, the expressions of gpbo_acq_argbest
 * A pivot a_jj that is not positive makes that candidate's mu, sd and ys NaN, and the selection's "first NaN wins" rule applies.  A
 * NaN candidate coordinate gives NaN too, and that candidate's row of nbr_out is -1.  A candidate's bits depend neither on M nor
 * on the other candidates.
 *
 * Outputs, selection and index_offset: gpls_sur_argbest's — best_idx / best_val the arg-best of ys, seed_idx / seed_val (k_seeds)
 * its argsort[:k_seeds], ys_out (M,) or NULL; the selection is gpbo_acq_argbest's own kernels.  mu_out, sd_out (M,) or NULL.
 * nbr_out (M, k) or NULL: the neighbours' row indices in the stated order.
 * On the device (csrc/nngp.hip, csrc/nngp_plan.h): a brute-force search, lane = candidate with its coordinates in registers, the
 * rows staged through LDS and read as broadcasts, each candidate's current k-list of (d2, index) in LDS; then a batched k x k
 * Cholesky, one wave per 64 / k candidates with lane = row and the triangle in LDS.
 * A reader: no model slot, no resident mu / sd, not the candidates and not the negative-variance flag are touched; only the
 * context's acquisition values are overwritten.
 * Errors, in this order.  GPBO_ERR_INVALID: k not 16, 32 or 64; N outside [k, GPNN_MAX_N]; d outside [1, GPBO_MAX_DIM]; n_ls not 1 or
 * d.  GPBO_ERR_UNSUPPORTED: a kernel kind outside the four; an acquisition kind outside the four.  GPBO_ERR_INVALID: NULL X, y_norm
 * or length_scale; a length scale not positive and finite; amplitude not positive and finite, white or alpha negative or not finite;
 * kappa_or_xi or y_max not finite; y_std not finite or not positive, y_mean not finite; k_seeds outside [0, GPBO_MAX_SEEDS]; a NULL
 * best_idx / best_val (seed_idx / seed_val with k_seeds > 0); an entry of X or y_norm not finite.  GPBO_ERR_STATE: no resident
 * candidates, or candidates whose dimension is not d.  GPBO_ERR_HIP: an allocation that fails.  There is no group or communicator
 * form. */
int gpnn_acq_argbest(gpbo_ctx* ctx, const double* X, const double* y_norm, int64_t N, int d, int kernel, const double* length_scale,
                     int n_ls, double amplitude, double white, double alpha, int k, int acq, double kappa_or_xi, double y_max,
                     double y_mean, double y_std, int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val,
                     int64_t* seed_idx, double* seed_val, double* ys_out, double* mu_out, double* sd_out, int64_t* nbr_out);

#ifdef GPBO_DEBUG
/* debug library only.  Kernel milliseconds (HIP events) of the four stages of the context's last gpnn_acq_argbest: ms[0] upload and
 * scaling, ms[1] the neighbour search, ms[2] the local solves, ms[3] the selection. */
int gpnn_debug_stage_ms(gpbo_ctx* ctx, float* ms);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GPNN_H */
