/* gpls.h — level-set estimation over the resident candidates: the SUR excursion-set acquisition, exported by libgpbo.so next to the C
 * ABI of gpbo.h.
 *
 * A header of its own for the reason gpiv.h is: the library's gpbo_ exports are exactly what gpbo.h declares, and each of its
 * functions is classified by a closed table of the order-of-calls contract.  The call is declared here under the prefix gpls_.
 * gpbo.h supplies gpbo_ctx, the status codes and the limits; GPBO_ABI_VERSION does not change, because nothing in gpbo.h changes
 * meaning.  Valid C99 on its own.  The function is a reader in the order-of-calls sense. */
#ifndef GPLS_H
#define GPLS_H

#include "gpbo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPLS_MAX_POINTS 4096

/* Stepwise uncertainty reduction for the excursion set {x : f(x) > level} (Bect, Ginsbourger, Li, Picheny & Vazquez 2012; closed
 * form: Chevalier, Bect, Ginsbourger, Vazquez, Picheny & Richet 2014).  Every other acquisition of gpbo.h asks about the optimum,
 * gpiv_ivr_argbest about the surrogate everywhere; this one asks where the function crosses a level: the boundary of a feasible
 * region, a failure domain, a contour to map.  Among J integration points a_j the classification uncertainty is
 * sum_j omega_j p_j (1 - p_j), p_j = P(f(a_j) > level); a candidate x is worth the expected drop of that sum after ONE noisy
 * observation at x.
 * In normalised units, as gpiv.h: c slot 0's amplitude, w its white noise, eta the value on the fit's diagonal, lambda = c eta, v(x) =
 * (sd(x) / y_std)^2 from slot 0's resident posterior, alpha the fit's weights.  Per point, once:
 *   V_j      = -K'^-1 k*(a_j)
 *   m_j      = sum_i alpha_i k*(a_j)_i                          the 256 strided partial sums i = t, t + 256, ... by a fixed tree
 *   s_j^2    = c max(1 + sum_i k*(a_j)_i V_j,i, 0)              latent variance at a_j, the same order
 *   t        = (level - y_mean) / y_std
 *   h_j      = (m_j - t) / s_j,                                 p_j = Phi(h_j)
 * per (candidate, point), cov_j(x) and den2(x) EXACTLY gpiv_ivr_argbest's (same V_j, same order of sums, same bits):
 *   r2       = min(cov_j(x)^2 (1 / den2(x)) (1 / s_j^2), 1)     squared correlation of the observation at x with f(a_j)
 * Chevalier's term E[p+ (1 - p+)] is Phi2(h_j, -h_j; rho = -r2), and Plackett's identity turns the expected reduction into one smooth
 * integral, taken here in the half-angle variable u = tan(theta / 2) so that neither asin nor sin is needed:
 *   G(h^2, r2) = Phi(h) Phi(-h) - Phi2(h, -h; -r2) = (1 / 2 pi) int_0^{asin r2} exp(-h^2 / (1 + sin theta)) d theta
 *              = (1 / pi) int_0^U exp(-h^2 (1 + u^2) / (1 + u)^2) / (1 + u^2) du,      U = r2 / (1 + sqrt((1 - r2) (1 + r2)))    >= 0
 *   SUR(x)   = sum_j omega_j G(h_j^2, r_j(x)^2)                 in [0, sum_j omega_j p_j (1 - p_j)];       ys = -SUR
 * The integral is a 12-node Gauss-Legendre rule on [0, U], nodes ascending (csrc/sur_plan.h): within 2e-15 absolute of the integral
 * for every h and every r2 in [0, 1]; at r2 = 1 it is Phi(h) Phi(-h), the point's whole uncertainty.
 * omega = weights (J,), or 1 / J each when weights is NULL; weights of the caller's own are used as given.
 * Conventions.  s_j == 0: the point is decided, its term is 0 and p_j is 1 where m_j > t, else 0.  den2(x) == 0: nothing is
 * learned, 0.  r2 == 0: exactly 0.  A NaN mu(x), sd(x) or candidate coordinate: NaN, and the selection's "first NaN wins" rule applies.
 * fp64 whatever the slot's precision.  Every sum has a fixed order — cov_j(x) as gpiv.h states; the nodes ascending; the column
 * fragments of a wave in order and the 16 columns of a fragment by a butterfly; the four waves in order; the column tiles in order
 * (csrc/sur.hip) —, and a candidate's bits depend neither on M nor on the other candidates.
 * points (n_points, d): host, parameter space, finite.  level: raw target units.  y_mean, y_std: those of the posterior pass that
 * left mu / sd.
 * Outputs, selection and index_offset: gpiv_ivr_argbest's — best_idx / best_val the arg-best of ys, seed_idx / seed_val (k_seeds) its
 * argsort[:k], ys_out (M,) or NULL.  p_out (n_points,) or NULL: p_j.  unc_out (1,) or NULL: sum_j omega_j p_j (1 - p_j), j ascending:
 * the uncertainty the scores are reductions of, the caller's stopping quantity.
 * On the device (csrc/sur.hip): gpiv's (M x N) (N x J) product on v_mfma_f64_16x16x4_f64 with k* generated into LDS, and behind each
 * column tile the quadrature per accumulator entry in registers; nothing of size M x J exists.  Workspace: the context's own,
 * O(J NP) doubles (csrc/sur_plan.h), grown on demand and kept; an allocation that fails is GPBO_ERR_HIP.
 * A reader, as gpiv_ivr_argbest: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates
 * and the negative-variance flag stay as they were; only the context's acquisition values are overwritten.
 * Errors, in this order.  GPBO_ERR_INVALID: n_points outside [1, GPLS_MAX_POINTS]; d outside [1, GPBO_MAX_DIM]; NULL points; a point
 * not finite; a weight that is NaN, infinite or negative, or weights whose sum is not positive; level not finite; k_seeds outside
 * [0, GPBO_MAX_SEEDS]; a NULL output; y_std not finite or not positive, y_mean not finite.  GPBO_ERR_STATE: a fit pending on slot 0,
 * slot 0 not fitted.  GPBO_ERR_INVALID: d not the model's.  GPBO_ERR_STATE: no resident posterior of slot 0 over the candidates.
 * GPBO_ERR_INVALID: y_std not the one that posterior was scaled with.  There is no group or communicator form. */
int gpls_sur_argbest(gpbo_ctx* ctx, const double* points, const double* weights, int n_points, int d, double level, double y_mean,
                     double y_std, int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val, int64_t* seed_idx,
                     double* seed_val, double* ys_out, double* p_out, double* unc_out);

#ifdef GPBO_DEBUG
/* debug library only.  Kernel milliseconds (HIP events) of the three stages of the context's last gpls_sur_argbest: ms[0] the points
 * (k*, solves, scalars, packing), ms[1] the scores, ms[2] the selection. */
int gpls_debug_stage_ms(gpbo_ctx* ctx, float* ms);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GPLS_H */
