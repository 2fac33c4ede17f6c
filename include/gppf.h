/* gppf.h — Pareto-frontier entropy search over the resident candidates, exported by libgpbo.so next to the C ABI of gpbo.h.
 *
 * A header of its own for the reason gpiv.h, gpje.h and gpla.h are: the library's gpbo_ exports are exactly what gpbo.h declares.
 * The call is declared here under the prefix gppf_.  gpbo.h supplies gpbo_ctx, the status codes and the limits; GPBO_ABI_VERSION
 * does not change, because nothing in gpbo.h changes meaning.  Valid C99 on its own.  The function is a reader in the
 * order-of-calls sense. */
#ifndef GPPF_H
#define GPPF_H

#include "gpbo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPPF_MAX_SAMPLES 64
#define GPPF_MAX_FRONT 128 /* = GPBO_MAX_QNEHVI_FRONT */
#define GPPF_MAX_FRONT_CANDIDATES 16384

/* Pareto-frontier entropy search for m = 2 (Suzuki, Takeno, Tamura, Shitara & Karasuyama 2020, "Multi-objective Bayesian
 * optimization using Pareto-frontier entropy"), in closed form: how much knowing that the observation at candidate x is dominated
 * by a sampled Pareto front lowers the entropy of that observation, averaged over S sampled fronts.  The information-theoretic
 * alternative to gpbo_ehvi_argbest: no reference point.
 * Objectives j = 0, 1 are slots 0, 1, both maximised, with independent posteriors Y_j ~ N(mu_j(x), sd_j(x)^2) taken from each
 * slot's resident mu / sd exactly as gpbo_ehvi_argbest reads them.  Front s has n_s points (a_k, c_k), k = 1 .. n_s, stored as
 * gpbo_qnhvi_greedy stores a front: objective 0 DESCENDING, so objective 1 strictly ascends.  With a_{n+1} = -inf the region front
 * s dominates is the disjoint union of the strips k = 1 .. n_s: (a_{k+1}, a_k] x (-inf, c_k].
 * Per candidate and draw, with z0_k = (a_k - mu_0) / sd_0 and z1_k = (c_k - mu_1) / sd_1 (true divisions):
 *   t = erfc(|z| / sqrt2) / 2;   z < 0: L = t, U = 1 - t;   z >= 0: U = t, L = 1 - t;   psi = z phi(z)
 *                                                                      (level -inf: L = 0, U = 1, psi = 0)
 *   P0_k = (z0_{k+1} >= 0) ? U0_{k+1} - U0_k : L0_k - L0_{k+1}         mass of strip k along objective 0, no cancellation in either tail
 *   G0_k = psi0_{k+1} - psi0_k                                         l phi(l) - u phi(u)
 *   P1_k = L1_k,   G1_k = -psi1_k
 *   Z_s  = sum_k P0_k P1_k
 *   Q_s  = sum_k (G0_k P1_k + P0_k G1_k)
 *   a_s(x) = -log Z_s - Q_s / (2 Z_s)                                  = H[p(y)] - H[p(y | y dominated by front s)]; the sd terms cancel
 *   a(x) = (a_0 + ... + a_{S-1}) / S,      ys = -a(x)
 * a is in nats.  With n_s = 1 it is the sum of two gpbo_mes_argbest terms, -log Phi(g_j) + g_j phi(g_j) / (2 Phi(g_j)).
 * Order of the sums.  Z_s and Q_s run k ascending into one accumulator each, from 0; the mean runs s ascending into one
 * accumulator from 0, followed by ONE true division by S.  No multiply-add is fused.  A candidate's bits depend on S and on the
 * fronts, and neither on M, nor on the launch geometry, nor on the other candidates.
 * Conventions.  sd_j == 0: L is the step [level >= mu_j], U its complement, psi = 0.  A NaN mu or sd of either objective: NaN, and
 * the selection's "first NaN wins" rule applies.  phi(z) == 0 (|z| beyond ~38.6): psi = 0.  LIMITATION: a draw whose Z_s is below
 * DBL_MIN (0 included) contributes a_s = 0, never NaN or +-inf — such a candidate sits tens of sd beyond the whole sampled front,
 * where the true value grows without bound; a front of no points (device-front mode over draws that are NaN everywhere) is this
 * case for every candidate.  fp64 whatever a slot's precision.
 *
 * Host-front mode (omega == NULL).  S = n_samples in [1, GPPF_MAX_SAMPLES]; front_size_in (S,), each in [1, GPPF_MAX_FRONT];
 * fronts_in (S, GPPF_MAX_FRONT, 2), point k of front s = (a, c) in raw target units, rows past a front's size not read.  Every
 * front must be finite with objective 0 strictly descending and objective 1 strictly ascending.  n_groups, n_paths, n_features,
 * phase, weights, eps and y_mean's values are not looked at.
 * Device-front mode (omega != NULL).  S = n_groups n_paths <= GPPF_MAX_SAMPLES; omega, phase, weights, eps are laid out as
 * gpbo_qnhvi_greedy lays them out for two slots (slot-major, then group-major); n_samples, front_size_in and fronts_in are not
 * looked at.  Joint draw t = g n_paths + s of both objectives is evaluated at the first B = min(M, GPPF_MAX_FRONT_CANDIDATES)
 * resident candidates by the evaluator the candidates get in gpbo_sample_paths — the same bits —, and every draw's front is built
 * on the device by gpbo_qnhvi_greedy's front rule without a reference point: every pair of two values that are neither NaN nor
 * -inf counts; equal pairs count once.  A front of more than GPPF_MAX_FRONT points is GPBO_ERR_UNSUPPORTED, as there; a front is
 * never thinned.
 * y_mean, y_std (2,): those of the posterior passes that left mu / sd.  front_size_out (S,), fronts_out (S, GPPF_MAX_FRONT, 2) or
 * NULL: the fronts actually scored (rows past a front's size unspecified).
 * Outputs, selection and index_offset: gpbo_mes_argbest's on the key ys.
 * On the device (csrc/pfes.hip, csrc/pfes_plan.h): lane = candidate, four waves on the same 64 candidates with the draws dealt
 * over the waves, the fronts staged in LDS 16 draws at a time and read as wave-wide broadcasts, (L, U, psi) of a strip's lower
 * level carried in registers into the next strip — one new level per objective per strip and no per-candidate level table.
 * Workspace: the context's own, O(S (B + GPPF_MAX_FRONT)) doubles, grown on demand and kept.
 * A reader, as gpje_jes_argbest: the slots' fits, their resident mu / sd, what gpbo_posterior_refresh may still refresh, the
 * candidates and the negative-variance flag stay as they were; only the context's acquisition values are overwritten.
 * Errors, in this order.  GPBO_ERR_INVALID: host-front mode: n_samples outside [1, GPPF_MAX_SAMPLES], NULL front_size_in or
 * fronts_in; device-front mode: n_groups outside [1, 16], n_paths outside [1, 16], n_features outside [1, 4096], n_groups n_paths
 * above GPPF_MAX_SAMPLES, NULL phase, weights or eps; then k_seeds outside [0, GPBO_MAX_SEEDS]; NULL y_mean, y_std or a NULL
 * output; a y_std not finite or not positive, a y_mean not finite; host-front mode: a front size outside [1, GPPF_MAX_FRONT], a
 * front that is not finite, whose objective 0 does not strictly descend or whose objective 1 does not strictly ascend.
 * GPBO_ERR_STATE: a fit pending on slot 0 or 1, slot 0 or 1 not fitted (slot 0 first); no candidates; no resident posterior of
 * both slots over them.  GPBO_ERR_INVALID: a y_std not the one its slot's posterior was scaled with.  GPBO_ERR_UNSUPPORTED: device-front mode, a front beyond GPPF_MAX_FRONT points (nothing is
 * scored).  There is no group or communicator form. */
int gppf_pfes_argbest(gpbo_ctx* ctx, const double* y_mean, const double* y_std, int n_groups, int n_paths, int n_features,
                      const double* omega, const double* phase, const double* weights, const double* eps, int n_samples,
                      const int* front_size_in, const double* fronts_in, int k_seeds, int64_t index_offset, int64_t* best_idx,
                      double* best_val, int64_t* seed_idx, double* seed_val, double* ys_out, int* front_size_out, double* fronts_out);

#ifdef GPBO_DEBUG
/* debug library only.  Kernel milliseconds (HIP events) of the three stages of the context's last gppf_pfes_argbest: ms[0] the
 * draws and the fronts (host-front mode: the fronts' upload), ms[1] the scores, ms[2] the selection. */
int gppf_debug_stage_ms(gpbo_ctx* ctx, float* ms);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GPPF_H */
