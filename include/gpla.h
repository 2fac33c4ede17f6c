/* gpla.h — two-step lookahead expected improvement over the resident candidates, exported by libgpbo.so next to the C ABI of gpbo.h.
 *
 * A header of its own for the reason gpiv.h and gpje.h are: the library's gpbo_ exports are exactly what gpbo.h declares.  The call
 * is declared here under the prefix gpla_.  gpbo.h supplies gpbo_ctx, the status codes and the limits; GPBO_ABI_VERSION does not
 * change, because nothing in gpbo.h changes meaning.  Valid C99 on its own.  The function is a reader in the order-of-calls sense. */
#ifndef GPLA_H
#define GPLA_H

#include "gpbo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPLA_MAX_POINTS 64
#define GPLA_MAX_NODES 32

/* Two-step lookahead expected improvement (Ginsbourger & Le Riche 2010; Wu & Frazier 2019, "Practical two-step look-ahead Bayesian
 * optimization"; qMultiStepLookahead with one fantasy stage of EI): the improvement the observation at candidate x brings now, plus
 * the best expected improvement left over x itself and J reference points once that observation has been absorbed, in expectation
 * over the observation by a quadrature rule the caller supplies (Gauss-Hermite: nodes z_h of the standardised observation, weights
 * omega_h summing to 1).  Closed form per (candidate, node, point); no Monte Carlo.  The non-myopic acquisition for near-noiseless
 * objectives, where gpbo_kg_argbest looks ahead at the posterior mean for noisy ones.
 * In normalised units, as gpbo_kg_argbest and gpje_jes_argbest: c the slot's amplitude, w its white noise, eta the value on the
 * fit's diagonal, lambda = c eta (from the slot), everything from slot 0's resident posterior.  Per point a_j, j = 1 .. J, once:
 *   V_j = -K'^-1 k*(a_j)
 *   m_j = sum_i alpha_i k(a_j, X_i)                          mu_points_out[j - 1] = y_std m_j + y_mean
 *   p_j = max(c (1 + sum_i k(a_j, X_i) V_j,i), 0)            var_points_out[j - 1] = y_std^2 p_j   (both sums: 256 strided partial sums, a tree)
 * Per candidate x:
 *   v = (sd(x) / y_std)^2,  vl = max(v - w, 0),  vo = (v + lambda) - w,  den = sqrt(vo)
 *   mn = (mu(x) - y_mean) / y_std,  bn = (y_best - y_mean) / y_std
 *   cov_j = c (k(x, a_j) + sum_i k(x, X_i) V_j,i)           j = 1 .. J
 *   point 0 is x itself: m_0 = mn, p_0 = vl, cov_0 = vl
 *   g_j = cov_j / den                                       the slope of point j's mean in the standardised observation
 *   q_j = sqrt(max(p_j - g_j g_j, 0))                       the latent sd at point j AFTER the observation: the same at every node
 *   e1  = G(mn, den, bn)                                    G(mean, sd, a) = E[(Y - a)^+], Y ~ N(mean, sd^2)
 *   per node h = 0 .. H - 1:
 *     b_h = max(bn, mn + den z_h)                           the incumbent after observing y_h
 *     t_h = max over j = 0 .. J of G(m_j + g_j z_h, q_j, b_h)        j ascending; a NaN term makes t_h NaN
 *   a(x) = e1 + sum_h omega_h t_h                           h ascending into one accumulator that starts at e1;     ys = -(y_std a)
 * a is in raw target units and >= plain EI at x, since every t_h >= 0.
 * G over its ranges, z = (mean - a) / sd, as gpbo_ehvi_argbest evaluates E[(Y - a)^+]: z > -1 sd (phi(z) + z Phi(z)), Phi and phi as
 * gpbo_acq_argbest's EI has them; z <= -1 sd phi(z) r(z) with log EI's r = 1 + z Phi / phi (erfcx down to -28, the series below),
 * 0 where phi underflows; sd == 0: max(mean - a, 0).
 * There is no xi: the exploration margin of this acquisition is the look-ahead itself.
 * Order of cov_j's sum: gpje_jes_argbest's, with J in S's place.  J <= 16: four partial sums, partial q over the train points i with
 * (i mod 32) / 8 == q; 16 < J <= 32: two, over (i mod 32) / 16; J > 32: one.  Inside a partial i ascends by the matrix core's k-steps
 * of four; k(x, a_j) is the last term of the LAST partial; the partials are added in order.  So a candidate's bits depend on J through
 * this split and on H, and neither on M, nor on the grid, nor on the other candidates.
 * Conventions.  den == 0: every g_j = 0 and e1 = max(mn - bn, 0) — nothing is learned, and the second step is the best one-step EI
 * over the points.  A NaN mu(x), sd(x) or candidate coordinate: NaN, and the selection's "first NaN wins" rule applies.  fp64 whatever
 * the slot's precision.
 * points (n_points, d): host, parameter space, finite.  nodes, weights (n_nodes,): host; finite, the weights >= 0 and not all 0 — the
 * device does not care where they come from (numpy.polynomial.hermite_e.hermegauss with the weights divided by sqrt(2 pi) is the
 * Gauss-Hermite rule of a unit normal).  y_best: the incumbent in raw target units, finite.  y_mean, y_std: those of the posterior
 * pass that left mu / sd.  mu_points_out, var_points_out (n_points,) or NULL.
 * Outputs, selection and index_offset: gpbo_mes_argbest's on the key ys.
 * On the device (csrc/lookahead.hip): gpje_jes_argbest's (M x N) (N x J) product on v_mfma_f64_16x16x4_f64 with k* generated into
 * LDS, and behind it, from LDS, an epilogue in three phases — g_j and q_j per (candidate, point), t_h per (candidate, node) with the
 * nodes dealt over the workgroup's four waves, the weighted sum per candidate (csrc/lookahead_plan.h has the LDS budget); nothing of
 * size M x J or M x H exists in memory.  Workspace: the context's own, O(J NP) doubles, grown on demand and kept.
 * A reader, as gpje_jes_argbest: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates
 * and the negative-variance flag stay as they were; only the context's acquisition values are overwritten.
 * Errors, in this order.  GPBO_ERR_INVALID: n_points outside [1, GPLA_MAX_POINTS]; n_nodes outside [1, GPLA_MAX_NODES]; d outside
 * [1, GPBO_MAX_DIM]; NULL points, nodes or weights; a point not finite; a node not finite; a weight not finite; a negative weight, or
 * all weights zero; y_best not finite; k_seeds outside [0, GPBO_MAX_SEEDS]; a NULL output; y_std not finite or not positive, y_mean
 * not finite.  GPBO_ERR_STATE: a fit pending on slot 0, slot 0 not fitted.  GPBO_ERR_INVALID: d not the model's.  GPBO_ERR_STATE: no
 * resident posterior of slot 0 over the candidates.  GPBO_ERR_INVALID: y_std not the one that posterior was scaled with.  There is no
 * group or communicator form. */
int gpla_ei2_argbest(gpbo_ctx* ctx, const double* points, int n_points, int d, const double* nodes, const double* weights, int n_nodes,
                     double y_best, double y_mean, double y_std, int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val,
                     int64_t* seed_idx, double* seed_val, double* ys_out, double* mu_points_out, double* var_points_out);

#ifdef GPBO_DEBUG
/* debug library only.  Kernel milliseconds (HIP events) of the three stages of the context's last gpla_ei2_argbest: ms[0] the points
 * (k*, solves, m_j / p_j, packing), ms[1] the scores, ms[2] the selection. */
int gpla_debug_stage_ms(gpbo_ctx* ctx, float* ms);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GPLA_H */
