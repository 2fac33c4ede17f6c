/* gpmo3.h — batch noisy expected hypervolume improvement for THREE objectives, exported by libgpbo.so next to the C ABI of gpbo.h
 * and the constrained family of gpmo.h.
 *
 * A header of its own for the reason gpmo.h is one: the library's gpbo_ and gpmo_ exports are exactly what those two headers declare,
 * and each of their functions is classified by a closed table of the order-of-calls contract.  The three-objective call is declared
 * here under the prefix gpmo3_ and held to the same export contract by tests/test_qnehvi3_host.py.  gpbo.h supplies gpbo_ctx, the
 * status codes and the limits; GPBO_ABI_VERSION does not change, because nothing in gpbo.h changes meaning.  Valid C99 on its own.
 * The function is a reader in the order-of-calls sense. */
#ifndef GPMO3_H
#define GPMO3_H

#include "gpbo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Batch noisy expected hypervolume improvement for m = 3 objectives, built greedily over the resident candidates from joint posterior
 * draws (Daulton, Balandat & Bakshy 2021, cached-draws form): what gpbo_qnhvi_greedy does for two objectives.
 * Slots and inputs.  Objective j is slot j, j < 3, all MAXIMISED and fitted with the candidates' d; N, kernel kind, length scales,
 * scale and precision may differ.  y_mean / y_std / ref (3,).  T = G S draws, G = n_groups <= GPBO_MAX_QNEI_GROUPS, S = n_paths <=
 * GPBO_MAX_PATHS, F = n_features.  The inputs are gpbo_qnhvi_greedy's, concatenated in slot order 0, 1, 2: omega (3, G, F, d), phase
 * (3, G, F), weights (3, G, S, F), eps = slot j's (G, S, N_j) block, one after another.  Draw t = g S + s of slot j is
 * gpbo_sample_paths' f_s for slot j and group g's inputs, the same bits.  base (n_base, d): the observed points, then the pending ones.
 * Front.  P_t: the distinct triples of draw t at the base points that are strictly above ref in all three objectives, hold no NaN and
 * are not dominated (>= in all, > in one), STORED by objective 2 descending, then objective 0 descending, then objective 1 descending.
 * Cells.  A height-map sweep turns P_t (n points) into at most 2 n + 1 disjoint cells (x_lo, x_hi, y_lo, y_hi, h).  S is a staircase
 * in objectives (0, 1), objective 0 descending and objective 1 strictly ascending, empty at first.  For point (a, b, c) in stored
 * order: p = the number of points of S with objective 0 > a; [p, r) the run of S with objective 1 <= b; for k = p .. r the
 * rectangle x in (x_lo, x_hi], x_hi = a for k = p, else S[k-1].x, x_lo = S[k].x for k < |S|, else ref_0; y in (y_lo, b], y_lo =
 * S[k-1].y for k > 0, else ref_1; h = c — a rectangle with x_hi == x_lo is not stored —; then S[p, r) is replaced by (a, b).  After
 * the last point the ground: the strips of the final S, k ascending, x_hi = +inf for strip 0, y_hi = +inf, h = ref_2.
 * Score.  For draw t's values (f0, f1, f2) at candidate x a cell's term is (w+ v+) u+, w = min(f0, x_hi) - x_lo, v = min(f1, y_hi) -
 * y_lo, u = f2 - h, z+ = z where z > 0, else 0: TWO rounded products, no fused multiply-add.  HVI_t = the terms in emission order
 * into one accumulator from 0; NaN if f0, f1 or f2 is NaN.  key_j(x) = -((HVI_0 + ... + HVI_{T-1}) / T), t ascending from 0, ONE
 * division; +inf for a candidate picked earlier.  The pick is gpbo_acq_argbest's: the first NaN wins, else the least key, ties to the
 * lowest index.  A candidate's key bits do not depend on M, on the launch geometry or on the other candidates.
 * Update.  After a pick draw t's front absorbs y = (f0, f1, f2)_t(pick): unchanged if y has a NaN, is not strictly above ref in all
 * three, or is dominated by or equal to a point; else the points y dominates leave, y enters in its sorted place and the draw's cells
 * are rebuilt by the sweep.
 * Overflow.  A front of more than GPBO_MAX_QNEHVI_FRONT points, at the build or after an insertion, sets a device flag; the call
 * returns GPBO_ERR_UNSUPPORTED behind its one synchronisation and names the lowest such draw.  Nothing is thinned.
 * Outputs.  pick_idx, pick_gain (q,).  Optional (NULL: not fetched), block [0] before the first pick, block [1] after the last:
 * front_size_out (2, T) ints, fronts_out (2, T, GPBO_MAX_QNEHVI_FRONT, 3), cell_count_out (2, T) ints, cells_out
 * (2, T, 2 GPBO_MAX_QNEHVI_FRONT + 1, 5) — rows past a count unspecified —; values_out (3, T, M); base_values_out (3, T, n_base);
 * keys_out (q, M), every step's keys (a debugging aid: one copy per step).
 * On the device (csrc/qnehvi3.hip): the draws slot by slot and group by group through gpbo_sample_paths' kernels into a resident
 * (3, T, M) block; a workgroup per draw builds the front by repeated lexicographic arg-max over the live triples and one wave sweeps
 * it; per step a score kernel streams the block against the cells, staged in LDS in stages packed by the draws' cell counts
 * (csrc/qnehvi3_plan.h), the selection picks, and an update kernel with a wave per draw inserts and re-sweeps.  All q steps are
 * enqueued on the context's stream; the records and the optional outputs cross behind ONE synchronisation.  fp64 whatever a slot's
 * precision.
 * Workspace: the context's own (csrc/qnehvi3_plan.h) — the block 24 T M bytes (6 GiB at T = 256 and M = 2^20), 24 T n_base at the base
 * points, fronts 6144 T, cells 20560 T, the counts, the base points as given and scaled, the records 16 q, the flag 16 and the mask M
 * bytes —; grown on demand and kept; an allocation that fails is GPBO_ERR_HIP.
 * A reader, as gpbo_sample_paths: the fits, the resident mu / sd, what gpbo_posterior_refresh may still refresh, the candidates and
 * the negative-variance flag stay as they were; the context's acquisition values are overwritten.
 * Errors: gpbo_qnhvi_greedy's, in its order, over three slots — GPBO_ERR_INVALID: n_groups outside [1, GPBO_MAX_QNEI_GROUPS]; n_paths
 * outside [1, GPBO_MAX_PATHS] or n_features outside [1, GPBO_MAX_PATH_FEATURES]; a NULL y_mean / y_std / omega / phase / weights /
 * eps / ref / pick_idx / pick_gain; a y_std not finite or not positive, a y_mean or ref not finite; n_base outside
 * [0, GPBO_MAX_QNEHVI_BASE], n_base > 0 with a NULL or non-finite base; d not the slots'; q outside [1, GPBO_MAX_SEEDS], q > M.
 * GPBO_ERR_STATE: one of the slots 0, 1, 2 unfitted or with a fit pending, no resident candidates, candidates or a slot of another d.
 * There is no group or communicator form, and no constrained one. */
int gpmo3_nhvi_greedy(gpbo_ctx* ctx, const double* y_mean, const double* y_std,
                      int n_groups, int n_paths, int n_features,
                      const double* omega, const double* phase, const double* weights, const double* eps,
                      const double* ref, const double* base, int n_base, int d,
                      int q, int64_t index_offset,
                      int64_t* pick_idx, double* pick_gain,
                      int* front_size_out, double* fronts_out, int* cell_count_out, double* cells_out,
                      double* values_out, double* base_values_out, double* keys_out);

#ifdef GPBO_DEBUG
/* debug library only.  Kernel milliseconds of the last gpmo3_nhvi_greedy's stages: ms[0] the draws, ms[1] the front and cell build,
 * ms[2] the q greedy steps. */
int gpmo3_debug_stage_ms(gpbo_ctx* ctx, float* ms);

/* debug library only.  The front build and the sweep on host-given values, base_values (3, n_draws, n), then the update rule with
 * insert_values (3, n_draws, n_insert), in order.  front_size_out / cell_count_out (n_draws,), fronts_out (n_draws,
 * GPBO_MAX_QNEHVI_FRONT, 3), cells_out (n_draws, 2 GPBO_MAX_QNEHVI_FRONT + 1, 5).  n_draws in [1, 4096], n in [0,
 * GPBO_MAX_QNEHVI_BASE], n_insert in [0, 4096].  A front that outgrows its array is GPBO_ERR_UNSUPPORTED; the context stays usable.
 * Touches no model slot. */
int gpmo3_debug_cells(gpbo_ctx* ctx, int n_draws, int n, const double* base_values, const double* ref, int n_insert,
                      const double* insert_values, int* front_size_out, double* fronts_out, int* cell_count_out, double* cells_out);
#endif

#ifdef __cplusplus
}
#endif
#endif /* GPMO3_H */
