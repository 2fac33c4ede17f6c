// How a fit / log-marginal-likelihood evaluation is laid out and routed (gpbo_api.hip), as pure functions of plain values: the size
// tier, the Cholesky's outer panel width, the lane grouping of gpbo_lml_batch, what follows from the tier, and the buffer sizes of
// a model.  Host-only and free of HIP: tests/test_fit_plan_host.py compiles it with the system C++ compiler and pins the rule on
// both sides of every edge.  The debug switches (GPBO_FUSED_MAX_NP, GPBO_MID_MAX_NP, GPBO_CHOL_OUTER, GPBO_LML_PER_GROUP) are read
// by the caller and come in already parsed (NO_OVERRIDE: not set).  The Cholesky look-ahead rule is not here: chol_kernels.hip.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>

#include "gpbo.h"

namespace gpbo {

constexpr int NB = 64;                   // Cholesky / inverse block size (one MFMA GEMM tile edge); NP is a multiple of it
constexpr int NO_OVERRIDE = INT_MIN;     // a debug switch that is not set

// fused_small.hip: the whole fit / LML evaluation of a problem of NP <= fused_max_np() as one launch of one workgroup per model
constexpr int FUSED_NP_DEFAULT = 64, FUSED_NP_CAP = 512;
// mid_fit.hip: fused_max_np() < NP <= mid_max_np(): the strip algorithms, ~15 launches
constexpr int MID_NP_DEFAULT = 768, MID_NP_CAP = 1024;

// Largest padded size the fused kernel serves: 64 in the product.  (At NP = 128 — still one diagonal workgroup plus a handful of
// tiles — the strip path of mid_fit.hip is faster, 50 against 79 us per fit and 94 against 118 per LML + gradient; at NP = 64 the
// one launch wins the LML evaluation, 67 against 74 us, and loses 5 us on the fit: profiles/r05_small_fit_timing.json.  Debug
// build: GPBO_FUSED_MAX_NP = 0 / 64 / 128 / ... up to FUSED_NP_CAP, read per call, for the bitwise A/B tests and the crossover
// measurement.)
inline int fused_max_from(int override) { return std::min(override == NO_OVERRIDE ? FUSED_NP_DEFAULT : override, FUSED_NP_CAP); }

// Largest padded size the strip path serves (fused_max_np() < NP <= mid_max_np()).  The strip's LDS image caps it at 1024; the
// default (768) is where one lane stops beating the multi-launch path (profiles/r05_small_fit_timing.json: fit 0.31 vs 0.39 ms at
// 768, 0.44 vs 0.49 at 1024 but a resident lane 0.52 vs 0.51 there).  (Debug build:
// GPBO_MID_MAX_NP = 0 ... 1024 read per call, for the A/B tests and the crossover measurement.)
inline int mid_max_from(int override) { return std::min(override == NO_OVERRIDE ? MID_NP_DEFAULT : override, MID_NP_CAP); }

enum class FitTier {
  Fused,    // NP <= fused_max: ONE launch of one workgroup per model                       fused_small.hip
  Strip,    // fused_max < NP <= mid_max: quarter-tile K, W by column strips, ~15 launches   mid_fit.hip
  Blocked,  // beyond: K, blocked Cholesky, W by recursive doubling, alpha, ~60 launches     fit_kernels.hip, chol_kernels.hip
};
inline FitTier fit_tier(int64_t NP, int fused_max, int mid_max) {
  if (NP <= fused_max) return FitTier::Fused;
  return NP <= mid_max ? FitTier::Strip : FitTier::Blocked;
}

// What follows from the tier.
// May a lane group's launch sequence be captured into a hipGraph and replayed (gpbo_lml_batch)?  Blocked only: Fused is one
// launch for the whole group: nothing to capture
// ... and the strip path's ~17 launches are enqueued faster than the device runs them: replaying them from a graph bought nothing
// at a fixed shape (six lanes at N = 512: 0.292 ms replayed, 0.283 launched) and cost a maximize() loop — whose N grows by one
// per step, a new shape every call — ~1 ms of capture + instantiation per suggest() (profiles/r05_maximize_loop.json)
inline bool graph_eligible(FitTier t) { return t == FitTier::Blocked; }
// Where the K^-1 of the LML gradient is built (the tail behind a Strip or Blocked factorisation; the fused kernel has its own).
// true — small problems: K^-1 tile by tile inside the gradient launch (kinv_grad_kernel), the two LML terms in its final launch
// false — K^-1 = W^T W (lower tiles) into the K buffer, then the trace reduction; partials go to m.tmp
inline bool kinv_in_grad_launch(FitTier t) { return t != FitTier::Blocked; }

// Outer panel width of the blocked Cholesky (launch_cholesky128), a multiple of 2 * NB; anything else becomes 2 * NB.
inline int chol_outer(int64_t NP, int override = NO_OVERRIDE) {
  // Outer panel width by size (scripts/archive/r03_chol_probe.py, round-3 schedule): up to NP = 2048 one panel — the rank-128
  // updates of the steps reach the whole trailing matrix, whose traffic is still small, and no latency-bound
  // rank-`outer` GEMM stands between the steps (NP = 1024: 0.312 -> 0.283 ms, 2048: 0.683 -> 0.618); 1024 up to NP = 4096
  // (1.70 -> 1.66-1.68); 512 beyond (8192: 6.0 against 6.36 with 1024), where the trailing matrix no longer fits the
  // caches and every pass over it counts.
  int outer = NP <= 2048 ? (int)((NP + 2 * NB - 1) / (2 * NB) * (2 * NB)) : (NP <= 4096 ? 1024 : 512);
  if (override != NO_OVERRIDE) outer = override;
  if (outer < 2 * NB || outer % (2 * NB)) outer = 2 * NB;
  return outer;
}

// Lanes are processed in groups: a group runs the launch sequence once for its lanes on its own stream.  Small
// problems are dispatch-bound (every kernel is tiny): ONE group of all lanes.  From NP = 2048 on the big GEMMs fill
// the chip by themselves and what is left to win is hiding one lane's latency-bound steps (the diagonal-block
// kernels) behind another lane's GEMMs — which a SECOND stream does and a third does not: three lanes on three streams
// take what two take plus one alone (2.16 against 1.22 + 0.94 ms at N = 2048; it is not the hardware queues — four streams of
// one-workgroup kernels do run side by side, scripts/probes/stream_queues.hip — but what two evaluations in the same phase
// leave free of the chip).  So: two groups, and inside a group lane = a grid dimension, where the chain's launches are
// shared (the diagonal blocks of all its lanes factor side by side in one step launch).  Until round 6: one lane per group
// from NP = 2048 on.  profiles/r06_lanes_grouping.json, ms for 3 / 4 / 6 lanes:
//   N = 2048: one lane per group 2.16 / 2.36 / 2.72, two groups 1.48 / 1.72 / 2.25;  N = 3072: 4.01 / 4.63 / 5.78 -> 3.17 / 3.82 / 5.31
//   N = 4096: 5.59 / 8.33 / 11.14 -> (three lanes on three streams stay) / 7.19 / 10.01 with two lanes per group;  N = 6144: 21.5 -> 18.9 at 4
struct LaneGroups {
  int per_group;   // lanes of every group but (possibly) the last
  int n_groups;
};
inline LaneGroups lane_groups(int64_t NP, int n_theta, int override = NO_OVERRIDE) {
  int per_group = n_theta;
  if (NP >= 4096) per_group = (n_theta <= 3) ? 1 : 2;
  else if (NP >= 2048) per_group = (n_theta + 1) / 2;
  if (override != NO_OVERRIDE) per_group = std::max(1, std::min(override, n_theta));   // A/B runs (debug build)
  return {per_group, (n_theta + per_group - 1) / per_group};
}

// The buffers of a model, in doubles.  alloc_model allocates a slot's from this table; gpbo_lml_batch lays a lane of its slab out
// by it — every launcher addresses lane l as "the model's buffer + l * stride", so the two must agree.  (Wp, mu, sd, Wp32, Wd
// belong to slots only.)
enum FitBuf { FB_LS, FB_XS, FB_K, FB_L, FB_W, FB_DINV, FB_TMP, FB_YN, FB_TVEC, FB_ALPHA, FB_MODEL_COUNT,
              FB_SCAL = FB_MODEL_COUNT,   // lanes only: the reduction scratch of the lane's evaluation (ctx->red)
              FB_INFO,                    // lanes only: its pivot words (ctx->info_dev)
              FB_COUNT };
constexpr int64_t FIT_SCAL_DOUBLES = 8 + GPBO_MAX_DIM;   // what an evaluation needs of ctx->red
constexpr int64_t FIT_INFO_DOUBLES = 32;                  // FB_INFO: the pivot word first ...
constexpr int64_t FIT_INFO_PAIR = 2;                      // ... and a scaled lane's [eta, target scale] this many doubles behind it
static_assert(FIT_INFO_PAIR + 2 <= FIT_INFO_DOUBLES, "the lane's noise / target-scale pair leaves its info region");
struct FitBuffers { int64_t size[FB_COUNT]; };
inline FitBuffers fit_buffers(int64_t NP, int DP) {
  FitBuffers b{};
  b.size[FB_LS] = GPBO_MAX_DIM;
  b.size[FB_XS] = NP * DP;
  b.size[FB_K] = b.size[FB_L] = b.size[FB_W] = NP * NP;
  b.size[FB_DINV] = (NP / NB) * NB * NB;                                               // the inverted diagonal blocks
  b.size[FB_TMP] = std::max<int64_t>(NP * NP / 2, NP * (int64_t)GPBO_MAX_DIM);         // trtri's workspace | raw inputs (N, d)
  b.size[FB_YN] = b.size[FB_TVEC] = b.size[FB_ALPHA] = NP;
  b.size[FB_SCAL] = FIT_SCAL_DOUBLES;
  b.size[FB_INFO] = FIT_INFO_DOUBLES;
  return b;
}
// One lane of the slab: the buffers one behind the other, each rounded up to 32 doubles.
struct LaneSlab { int64_t off[FB_COUNT]; int64_t stride; };
inline LaneSlab lane_slab(const FitBuffers& b) {
  LaneSlab s{};
  for (int i = 0; i < FB_COUNT; ++i) {
    s.off[i] = s.stride;
    s.stride += (b.size[i] + 31) / 32 * 32;
  }
  return s;
}

}  // namespace gpbo
