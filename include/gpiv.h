/* gpiv.h — integrated posterior variance reduction over the resident candidates, exported by libgpbo.so next to the C ABI of gpbo.h.
 *
 * A header of its own for the reason gpmo.h and gpmo3.h are: the library's gpbo_ exports are exactly what gpbo.h declares, and each
 * of its functions is classified by a closed table of the order-of-calls contract.  The call is declared here under the prefix gpiv_.
 * gpbo.h supplies gpbo_ctx, the status codes and the limits; GPBO_ABI_VERSION does not change, because nothing in gpbo.h changes
 * meaning.  Valid C99 on its own.  The function is a reader in the order-of-calls sense. */
#ifndef GPIV_H
#define GPIV_H

#include "gpbo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPIV_MAX_POINTS 4096

/* Integrated posterior variance reduction (Cohn's ALC; IMSE-optimal design; qNegIntegratedPosteriorVariance at q = 1): how much ONE
 * noisy observation at candidate x lowers the latent posterior variance, summed with weights over J integration points a_j.  Every
 * other acquisition of gpbo.h asks about a candidate's own value, a draw's value there, or the maximum of the mean; this one asks
 * what the observation teaches about the surrogate over the whole box: active learning, calibration runs, the exploration phase of
 * a noisy campaign.
 * In normalised units, as gpbo_kg_argbest: c the slot's amplitude, w its white noise, eta the value on the fit's diagonal, lambda =
 * c eta (from the slot, not from the caller), v(x) = (sd(x) / y_std)^2 from slot 0's resident posterior:
 *   V_j      = -K'^-1 k*(a_j)                                  once per point
 *   cov_j(x) = c (k(x, a_j) + sum_i k(x, X_i) V_j,i)           i = 0 .. N - 1 in that order, k(x, a_j) last
 *   den2(x)  = (v(x) + lambda) - w
 *   IVR(x)   = y_std^2 (sum_j omega_j cov_j(x)^2) / den2(x)    >= 0, raw target units squared;       ys = -IVR
 * omega = weights (J,), or 1 / J each when weights is NULL: a Monte-Carlo estimate of the integrated reduction over the box when the
 * points are uniform draws.  Weights of the caller's own serve a measure that is not uniform; they are used as given.
 * Conventions.  den2 == 0: nothing is learned, 0.  A NaN mu(x), sd(x) or candidate coordinate: NaN, and the selection's "first NaN
 * wins" rule applies.  fp64 whatever the slot's precision.  Every sum has a fixed order — the train points by the matrix core's
 * k-steps of four, the columns of a wave by fragments of 16 and a butterfly inside one, the four waves in order, the column tiles in
 * order (csrc/ivr.hip) —, and a candidate's bits depend neither on M nor on the other candidates.
 * points (n_points, d): host, parameter space, finite.  y_mean, y_std: those of the posterior pass that left mu / sd.
 * Outputs, selection and index_offset: gpbo_kg_argbest's — best_idx / best_val the arg-best of ys, seed_idx / seed_val (k_seeds) its
 * argsort[:k], ys_out (M,) or NULL.
 * On the device (csrc/ivr.hip): an (M x N) (N x J) product on v_mfma_f64_16x16x4_f64 with k* generated into LDS and the squared,
 * weighted row sum behind it in registers; nothing of size M x J exists.  Workspace: the context's own, O(J NP) doubles
 * (csrc/ivr_plan.h), grown on demand and kept; an allocation that fails is GPBO_ERR_HIP.
 * A reader, as gpbo_kg_argbest: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates
 * and the negative-variance flag stay as they were; only the context's acquisition values are overwritten.
 * Errors, in this order.  GPBO_ERR_INVALID: n_points outside [1, GPIV_MAX_POINTS]; d outside [1, GPBO_MAX_DIM]; NULL points; a point
 * not finite; a weight that is NaN, infinite or negative, or weights whose sum is not positive; k_seeds outside [0, GPBO_MAX_SEEDS];
 * a NULL output; y_std not finite or not positive, y_mean not finite.  GPBO_ERR_STATE: a fit pending on slot 0, slot 0 not fitted.
 * GPBO_ERR_INVALID: d not the model's.  GPBO_ERR_STATE: no resident posterior of slot 0 over the candidates.  GPBO_ERR_INVALID: y_std
 * not the one that posterior was scaled with.  There is no group or communicator form. */
int gpiv_ivr_argbest(gpbo_ctx* ctx, const double* points, const double* weights, int n_points, int d, double y_mean, double y_std,
                     int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val,
                     double* ys_out);

#ifdef GPBO_DEBUG
/* debug library only.  Kernel milliseconds (HIP events) of the three stages of the context's last gpiv_ivr_argbest: ms[0] the points
 * (k*, solves, packing), ms[1] the scores, ms[2] the selection. */
int gpiv_debug_stage_ms(gpbo_ctx* ctx, float* ms);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GPIV_H */
