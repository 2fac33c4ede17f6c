/* gpje.h — joint entropy search over the resident candidates, exported by libgpbo.so next to the C ABI of gpbo.h.
 *
 * A header of its own for the reason gpiv.h is: the library's gpbo_ exports are exactly what gpbo.h declares.  The call is declared
 * here under the prefix gpje_.  gpbo.h supplies gpbo_ctx, the status codes and the limits; GPBO_ABI_VERSION does not change, because
 * nothing in gpbo.h changes meaning.  Valid C99 on its own.  The function is a reader in the order-of-calls sense. */
#ifndef GPJE_H
#define GPJE_H

#include "gpbo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPJE_MAX_SAMPLES 64

/* Joint entropy search, lower bound (Hvarfner, Hutter & Nardi 2022; Tu et al. 2022; qLowerBoundJointEntropySearch at q = 1): how much
 * observing candidate x lowers the entropy of the JOINT of the optimum's location and value.  gpbo_mes_argbest uses the sampled
 * maxima f*_s alone; this one uses the pairs (x*_s, f*_s) gpbo_ascend_paths returns: it conditions the GP on f(x*_s) = f*_s, truncates
 * f(x) at f*_s, and compares the observation's entropy before and after by moment matching.
 * In normalised units, as gpbo_kg_argbest: c the slot's amplitude, w its white noise, eta the value on the fit's diagonal, lambda =
 * c eta (from the slot), everything from slot 0's resident posterior.  Per sample s, once:
 *   V_s   = -K'^-1 k*(x*_s)
 *   m_s   = sum_i alpha_i k(x*_s, X_i)                      mu_star_out[s] = y_std m_s + y_mean
 *   p_s   = c (1 + sum_i k(x*_s, X_i) V_s,i)                var_star_out[s] = y_std^2 p_s      (both sums: 256 strided partial sums, a tree)
 *   fn_s  = (f_star[s] - y_mean) / y_std
 *   rho_s = 1 / p_s if p_s > 0, else 0                      a sample whose optimum sits on an observed point conditions nothing
 *   g_s   = rho_s (fn_s - m_s)
 * Per candidate x and sample s:
 *   v = (sd(x) / y_std)^2,  vl = max(v - w, 0),  vo = (v + lambda) - w,  mn = (mu(x) - y_mean) / y_std
 *   cov_s = c (k(x, x*_s) + sum_i k(x, X_i) V_s,i)
 *   mu_s  = mn + cov_s g_s
 *   vl_s  = max(vl - (cov_s cov_s) rho_s, 0)
 *   beta  = (fn_s - mu_s) / sqrt(vl_s)
 *   vt_s  = vl_s r2(beta),  r2(b) = 1 - b h - h^2,  h = phi(b) / Phi(b)
 *   a(x)  = 1/2 log(vo) - (sum_s 1/2 log(vt_s + lambda)) / S        s = 0 .. S - 1 in that order, one division;     ys = -a
 * The 2 pi e terms of the two entropies cancel.  a is in nats and >= 0 up to rounding.
 * Order of cov_s's sum.  S <= 16: four partial sums, partial q over the train points i with (i mod 32) / 8 == q; 16 < S <= 32: two,
 * over (i mod 32) / 16; S > 32: one.  Inside a partial i ascends by the matrix core's k-steps of four; k(x, x*_s) is the last term of
 * the LAST partial; the partials are added in order.  So a candidate's bits depend on S through this split, and neither on M nor on
 * the other candidates.
 * r2 over its ranges (x = -beta; relative error against mpmath, in fp64 NumPy / SciPy on the host: at most 1.8e-14, at beta just
 * above -2; the device is held to 4 x that, 7.1e-14, by tests/test_gpu_jes.py):
 *   beta >= -1        the formula as written, Phi and phi as gpbo_acq_argbest's EI evaluates them; 1 at +inf
 *   -2 < beta < -1    log EI's erfcx route: r = 1 + beta m, m = Phi / phi = (1 - r) / (-beta), r2 = 1 - r / m^2
 *   beta <= -2        Laplace's continued fraction of the Mills ratio, c_k = k / (x + c_k+1) from c_n+1 = 0: r2 = c_1 (c_2 - c_1),
 *                     n = 128 levels for x < 3, 64 for x < 6, 32 for x < 10, 16 from there on
 * and clamped into [0, 1]; NaN for a NaN beta.
 * Conventions.  vl_s == 0: the term is 1/2 log(lambda).  A NaN mu(x), sd(x) or candidate coordinate: NaN, and the selection's "first
 * NaN wins" rule applies.  lambda = 0 is not special-cased.  fp64 whatever the slot's precision.
 * x_star (n_samples, d): host, parameter space, finite.  f_star (n_samples,): raw target units, finite.  y_mean, y_std: those of the
 * posterior pass that left mu / sd.  mu_star_out, var_star_out (n_samples,) or NULL.
 * Outputs, selection and index_offset: gpbo_mes_argbest's on the key ys.
 * On the device (csrc/jes.hip): an (M x N) (N x S) product on v_mfma_f64_16x16x4_f64 with k* generated into LDS, the train points of
 * a stage split over the waves that share a 16-column fragment (csrc/jes_plan.h), the conditioning, r2 and the logs per (candidate,
 * sample) from LDS; nothing of size M x S exists in memory.  Workspace: the context's own, O(S NP) doubles, grown on demand and kept.
 * A reader, as gpiv_ivr_argbest: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates
 * and the negative-variance flag stay as they were; only the context's acquisition values are overwritten.
 * Errors, in this order.  GPBO_ERR_INVALID: n_samples outside [1, GPJE_MAX_SAMPLES]; d outside [1, GPBO_MAX_DIM]; NULL x_star or
 * f_star; an x_star not finite; an f_star not finite; k_seeds outside [0, GPBO_MAX_SEEDS]; a NULL output; y_std not finite or not
 * positive, y_mean not finite.  GPBO_ERR_STATE: a fit pending on slot 0, slot 0 not fitted.  GPBO_ERR_INVALID: d not the model's.
 * GPBO_ERR_STATE: no resident posterior of slot 0 over the candidates.  GPBO_ERR_INVALID: y_std not the one that posterior was scaled
 * with.  There is no group or communicator form. */
int gpje_jes_argbest(gpbo_ctx* ctx, const double* x_star, const double* f_star, int n_samples, int d, double y_mean, double y_std,
                     int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val,
                     double* ys_out, double* mu_star_out, double* var_star_out);

#ifdef GPBO_DEBUG
/* debug library only.  out[i] = the device's r2(beta[i]), i < n (host arrays). */
int gpje_debug_r2(gpbo_ctx* ctx, const double* beta, int n, double* out);
/* Kernel milliseconds (HIP events) of the three stages of the context's last gpje_jes_argbest: ms[0] the points (k*, solves, m_s /
 * p_s, packing), ms[1] the scores, ms[2] the selection. */
int gpje_debug_stage_ms(gpbo_ctx* ctx, float* ms);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GPJE_H */
