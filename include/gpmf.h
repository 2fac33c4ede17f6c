/* gpmf.h — multi-fidelity max-value entropy search over the resident candidates, exported by libgpbo.so next to the C ABI of gpbo.h.
 *
 * A header of its own for the reason gpje.h is: the library's gpbo_ exports are exactly what gpbo.h declares.  The call is declared
 * here under the prefix gpmf_.  gpbo.h supplies gpbo_ctx, the status codes and the limits; GPBO_ABI_VERSION does not change, because
 * nothing in gpbo.h changes meaning.  Valid C99 on its own.  The function is a reader in the order-of-calls sense. */
#ifndef GPMF_H
#define GPMF_H

#include "gpbo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPMF_MAX_SAMPLES 64

/* Multi-fidelity max-value entropy search, the GIBBON lower bound (Moss, Leslie & Rayson 2021; qLowerBoundMaxValueEntropy with a
 * fidelity column, at q = 1): how much a (noisy) observation at candidate z = (x, s), s its fidelity, tells about the maximum of
 * f(x, fid_target), per unit of cost.  One input column, fid_col, is the fidelity; a candidate row z has s = z[fid_col] in raw
 * parameter units, and z' is z with that column replaced by fid_target.  The call works from slot 0's FIT and the resident candidates
 * (M, d) alone; it needs no resident posterior and computes everything itself, the posterior COVARIANCE of f(z) and f(z') included.
 * In normalised units, as gpje_jes_argbest: c the slot's amplitude, lambda = c eta the observation noise (eta the value on the fit's
 * diagonal), alpha and W = L^-1 of the unit model, kappa the slot's kernel kind:
 *   k  = k*(z),  k' = k*(z')                 unit kernel against the N training points, every coordinate divided by its length scale
 *   u  = W k,    u' = W k'
 *   q  = sum u_i^2,  q' = sum u'_i^2,  x = sum u_i u'_i,  m' = sum alpha_i k'_i
 *   vl = c max(1 - q, 0)                     latent variance at z
 *   vg = c max(1 - q', 0)                    latent variance at z'            sd_t_out = y_std sqrt(vg)
 *   cv = c (kappa((s / l - fid_target / l)^2) - x)                            l the fidelity column's length scale
 *   vo = vl + lambda                         variance of the OBSERVATION at z
 *   rho^2 = min(cv^2 / (vo vg), 1) if vo > 0 and vg > 0, else 0               rho_out = sign(cv) sqrt(rho^2)
 *   gamma_s = ((y_star[s] - y_mean) / y_std - m') / sqrt(vg)                  mu_t_out = y_std m' + y_mean
 *   a  = -(sum_s log1p(-(rho^2 (1 - r2(gamma_s))))) / (2 S)                   s = 0 .. S - 1 in that order, one division
 *   ys = -a / (cost0 + cost1 s)
 * r2 is exactly gpje.h's (the same device function, its ranges and its error there).  a is in nats and >= 0 up to rounding.
 * Order of the sums.  A squared distance: the d - 1 other coordinates in column order (the fidelity column's place adds an exact
 * zero), one fma each, then the fidelity term of z, respectively of z', by one more fma.  u_i: the matrix core's k-steps of four
 * train points, ascending, up to the last column of row i's 16-row tile.  q, q', x: row i belongs to partial (wave, g) with g = i mod 4
 * and wave = t for t < 8, 15 - t otherwise, t = (i mod 256) / 16; inside a partial the 256-row chunks ascend, in a chunk tile `wave`
 * comes before tile 15 - wave, the rows of a tile ascend, one fma each; the four g of a wave add as (0 + 1) + (2 + 3), the eight
 * waves in order.  m': train point i belongs to partial i mod 16, ascending inside, one fma each; the sixteen partials add in order.
 * So a candidate's bits depend neither on M nor on the other candidates.
 * Conventions.  vg == 0 or vo == 0: a = 0.  A NaN coordinate: NaN, and the selection's "first NaN wins" rule applies.  A cost
 * cost0 + cost1 s that is not finite and positive: NaN.  lambda = 0 is not special-cased: a may then be +inf, which the selection
 * takes as the best key.  fp64 whatever the slot's precision.
 * y_star (n_samples,): host, raw target units, finite — the sampled maxima of f(., fid_target), e.g. gpbo_sample_paths' over points at
 * the target fidelity.  rho_out, mu_t_out, sd_t_out: (M,) or NULL.
 * Outputs, selection and index_offset: gpbo_mes_argbest's on the key ys.
 * On the device (csrc/mfmes.hip, csrc/mf_plan.h): ONE kernel on v_mfma_f64_16x16x4_f64.  A workgroup owns 32 candidates and walks
 * every 256-row chunk of W itself, so the three sums never leave it: no partials in memory, no second launch.  A stage's k and k'
 * come from one shared distance and lie in LDS as two B fragments over the same 16 candidates, so u and u' of a (row, candidate)
 * share a lane and their products are lane-local.  Workspace: the context's own, 64 + 3 M doubles at most, grown on demand and kept.
 * N: every N a slot can hold is served, above 16384 as below; nothing is refused by size but a grid beyond 2^31 - 1 tiles
 * (GPBO_ERR_UNSUPPORTED: shard the candidates).
 * A reader: the slot's fit, its resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates and the
 * negative-variance flag stay as they were; only the context's acquisition values are overwritten.
 * Errors, in this order.  GPBO_ERR_INVALID: n_samples outside [1, GPMF_MAX_SAMPLES]; NULL y_star; a y_star not finite; fid_col
 * outside [0, GPBO_MAX_DIM); fid_target not finite; cost0 not finite or <= 0; cost1 not finite or < 0; k_seeds outside
 * [0, GPBO_MAX_SEEDS]; a NULL output; y_std not finite or not positive, y_mean not finite.  GPBO_ERR_STATE: a fit pending on slot 0,
 * slot 0 not fitted, no candidates, candidates of another d than the model's.  GPBO_ERR_INVALID: fid_col not below the model's d
 * (only the fit knows d).  There is no group or communicator form. */
int gpmf_mes_argbest(gpbo_ctx* ctx, int fid_col, double fid_target, double cost0, double cost1, const double* y_star, int n_samples,
                     double y_mean, double y_std, int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val,
                     int64_t* seed_idx, double* seed_val, double* ys_out, double* rho_out, double* mu_t_out, double* sd_t_out);

#ifdef GPBO_DEBUG
/* debug library only.  Kernel milliseconds (HIP events) of the two stages of the context's last gpmf_mes_argbest: ms[0] the pair
 * pass, ms[1] the selection. */
int gpmf_debug_stage_ms(gpbo_ctx* ctx, float* ms);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GPMF_H */
