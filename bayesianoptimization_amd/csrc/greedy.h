// What the greedy draw batches share — gpbo_qnei_greedy and gpbo_cnei_greedy (qnei.hip), gpbo_qnhvi_greedy (qnehvi.hip) —, each
// thing once: the record of a pick and the rule that makes it, the loop of the q greedy steps, the layout of the draws' inputs, the
// records' way home, and the marks of the debug build's stage clock.  Needs HIP.  What differs stays with its file: the order of the draws'
// passes, the score and update kernels (a kernel cannot be launched from another translation unit: greedy_steps takes the launches
// as callables), and the workspace layouts (qnei_plan.h, cnei_plan.h, qnehvi_plan.h) inside the one buffer ctx->greedy.
#pragma once

#include "gpbo_internal.h"

#include <limits>

namespace gpbo {

struct GreedyRecord { double gain; int64_t idx; };
static_assert(sizeof(GreedyRecord) == 16, "a record is two doubles of the workspace");
static_assert(sizeof(GreedyRecord) * GPBO_MAX_SEEDS <= PIN_AUX_SEL_OUT_BYTES, "the picks' records outgrew the selection's pinned window");

// Behind a step's selection: the pick — the first NaN wins (as best_of_selection has it), else the selection's first pick.  local:
// its index among the M candidates, -1 where it lies outside them and touches nothing (never, with q <= M); gain and idx: the
// record's.
struct GreedyPick { int64_t local; bool nan; double gain; int64_t idx; };
__device__ __forceinline__ GreedyPick greedy_pick(const SelState* __restrict__ st, const Key* __restrict__ first, int64_t M,
                                                  int64_t offset) {
  const bool nan = st->first_nan != INT64_MAX;
  const int64_t pick = nan ? st->first_nan : first->i;
  const bool valid = pick >= 0 && pick < M;
  return {valid ? pick : -1, nan, (nan || !valid) ? std::numeric_limits<double>::quiet_NaN() : -first->v, valid ? pick + offset : -1};
}

// The q greedy steps, all on the stream: `score()` launches the caller's score kernel (the keys of step j into ctx->ys), then the
// selection's one pick, then `update(st, first, j)` launches the caller's update kernel behind it.
template <class Score, class Update>
int greedy_steps(gpbo_ctx* ctx, int64_t M, int q, double* keys_out, Score score, Update update) {
  int rc;
  for (int j = 0; j < q; ++j) {
    score();
    GPBO_HIP(ctx, hipGetLastError());
    if (keys_out)
      GPBO_HIP(ctx, hipMemcpyAsync(keys_out + (int64_t)j * M, ctx->ys, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    const SelState* st; const Key* first;
    if ((rc = enqueue_values_select(ctx, M, &st, &first))) return rc;
    update(st, first, j);
    GPBO_HIP(ctx, hipGetLastError());
  }
  return GPBO_OK;
}

// The draws' inputs as the entry points take them: omega (F, d), phase (F), weights (S, F) and eps (S, N_j) per (slot j, group g),
// concatenated slot-major, then group-major — so slot j's eps start behind the (G, S, N_i) blocks of the slots i < j.
struct GreedyDraws {
  int G, S, F, d;
  const double *omega, *phase, *weights, *eps;
  int64_t eps_at[GPBO_MAX_MODELS];
};
inline GreedyDraws greedy_draws(int n_slots, const Model* const* ms, int G, int S, int F, const double* omega, const double* phase,
                                const double* weights, const double* eps) {
  GreedyDraws dr{G, S, F, ms[0]->d, omega, phase, weights, eps, {}};
  int64_t at = 0;
  for (int j = 0; j < n_slots; ++j) { dr.eps_at[j] = at; at += (int64_t)G * S * ms[j]->N; }
  return dr;
}
// ... and group g of slot j (its model m) made resident in the paths workspace: launch_path_weights on the group's four inputs
inline int greedy_path_weights(gpbo_ctx* ctx, const GreedyDraws& dr, const Model& m, int j, int g, PathWorkspace* ws) {
  const int64_t jg = (int64_t)j * dr.G + g;
  return launch_path_weights(ctx, m, dr.S, dr.F, dr.omega + jg * dr.F * dr.d, dr.phase + jg * dr.F, dr.weights + jg * dr.S * dr.F,
                             dr.eps + dr.eps_at[j] + (int64_t)g * dr.S * m.N, 0, ws);
}

// The q records on their way home (enqueued; the caller synchronises): where they will stand on the host
template <class Record>
int greedy_fetch(gpbo_ctx* ctx, const Record* rec, int q, const Record** host) {
  static_assert(sizeof(Record) * GPBO_MAX_SEEDS <= PIN_AUX_SEL_ROOM, "the picks' records outgrew the room behind the selection's pinned window");
  Record* h = (Record*)((char*)ctx->pinned_aux + PIN_AUX_SEL_OUT);      // (behind the last selection: its records are read)
  GPBO_HIP(ctx, hipMemcpyAsync(h, rec, sizeof(Record) * (size_t)q, hipMemcpyDeviceToHost, ctx->stream));
  *host = h;
  return GPBO_OK;
}

// debug build: event i of the call's stage clock; the last one makes the clock readable (gpbo_api.hip: greedy_stage_ms reads it)
inline void greedy_mark(gpbo_ctx* ctx, StageClock& c, int i) {
#ifdef GPBO_DEBUG
  if (!c.ev[i]) (void)hipEventCreate(&c.ev[i]);
  (void)hipEventRecord(c.ev[i], ctx->stream);
  c.used = (i == c.n - 1);
#else
  (void)ctx; (void)c; (void)i;
#endif
}

}  // namespace gpbo
