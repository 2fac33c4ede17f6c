// How the posterior function draws are laid out and dispatched, as pure functions of plain values: the device workspace of
// gpbo_sample_paths / gpbo_ascend_paths (posterior_paths.hip: launch_path_weights fills its first part, path_ascent.hip:
// launch_path_ascent its second; both take every pointer from path_block), which instance of path_eval_kernel serves a call, and
// the two numbers both files need (the features' scale, the default iteration limit).  Free of HIP:
// tests/test_path_plan_host.py compiles it with the system C++ compiler and pins every offset and both sides of every edge.
#pragma once

#include <cmath>
#include <cstdint>

#include "gpbo.h"   // GPBO_MAX_PATHS

namespace gpbo {

constexpr int PATH_DEFAULT_MAX_ITER = 15000;      // gpbo_ascend_paths with max_iter < 0
constexpr int64_t PATH_EVAL_WIDE_M = 1 << 17;     // points from which path_eval_kernel runs 256 threads a workgroup

// accumulators path_eval_kernel holds per point: its NS instance for S paths
inline int path_eval_ns(int S) { return S == 1 ? 1 : (S <= 4 ? 4 : GPBO_MAX_PATHS); }
// as the refresh launcher: one workgroup per 256 points fills the device from ~2^17 points on; below, single-wave workgroups
inline unsigned path_eval_threads(int64_t M) { return M >= PATH_EVAL_WIDE_M ? 256u : 64u; }
// fs of g_s(x) = fs sum_j weights[s, j] cos(...): F features of a kernel of that amplitude
inline double path_feature_scale(double amplitude, int F) { return std::sqrt(2.0 * amplitude / (double)F); }

// The workspace (ctx->paths), offsets in doubles from its start:
//   omega (F, d) | phase (F) | weights (S, F) | eps (S, N) | G [S][NP] | T [S][NP] | V [S][NP]
// and, for the R = n_runs runs of an ascent (n_runs = 0: none, the block ends behind V),
//   lo (d) | hi (d) | starts (R, d) | x (R, d) | g (R, d) | f (R) | start_idx (R int64) | status (R ints) | evals (R ints)
// status and evals are offsets in INTS.  Each of the two has a full R doubles: R ints of slack follow status, and again evals.
struct PathBlock {
  int64_t omega, phase, weights, eps, G, T, V, lo, hi, starts, x, g, f, start_idx;
  int64_t status, evals;      // in ints
  int64_t doubles;
};
inline PathBlock path_block(int S_, int F_, int N_, int NP_, int d_, int n_runs) {
  const int64_t S = S_, F = F_, N = N_, NP = NP_, d = d_, R = n_runs, da = n_runs ? d_ : 0;
  PathBlock b{};
  b.omega = 0;
  b.phase = b.omega + F * d;
  b.weights = b.phase + F;
  b.eps = b.weights + S * F;
  b.G = b.eps + S * N;
  b.T = b.G + S * NP;
  b.V = b.T + S * NP;
  b.lo = b.V + S * NP;
  b.hi = b.lo + da;
  b.starts = b.hi + da;
  b.x = b.starts + R * d;
  b.g = b.x + R * d;
  b.f = b.g + R * d;
  b.start_idx = b.f + R;
  b.status = 2 * (b.start_idx + R);
  b.evals = 2 * (b.f + 3 * R);
  b.doubles = b.f + 4 * R;
  return b;
}

// gpbo_sample_paths_constrained: what path_eval_kernel does with a point's S values behind its accumulators.  PLAIN stores them
// (gpbo_sample_paths); a constraint slot folds its violation terms into viol[S][M] — the first one writes, the later ones add, so
// the sum's order is the slots' —; the objective reads viol and stores the selection key.  PATH_MASKED (gpbo_cnei_greedy's objective
// pass) reads viol as PATH_KEY does and stores the masked VALUE: f where the point is feasible, -inf where it is not, NaN kept.
enum PathEpilogue : int { PATH_PLAIN = 0, PATH_VIOL_WRITE = 1, PATH_VIOL_ADD = 2, PATH_KEY = 3, PATH_MASKED = 4 };
inline int path_epilogue(int slot) { return slot == 0 ? PATH_KEY : (slot == 1 ? PATH_VIOL_WRITE : PATH_VIOL_ADD); }

// Its own workspace (ctx->cpaths), offsets in doubles from its start:
//   viol [S][M] | vals [S][M] (only with values_out: one slot's values at a time, on their way to the host) |
//   pts [GPBO_MAX_PATHS][DP] | f [S][GPBO_MAX_PATHS]
// pts / f: the scaled candidates the rows WITHOUT a feasible candidate picked, and all S paths evaluated there again (row s reads
// its own).  Every part starts at an even offset: the kernel reads points as double2.
struct ConstrainedBlock { int64_t viol, vals, pts, f, doubles; };
inline ConstrainedBlock constrained_block(int S_, int64_t M, int DP, bool values) {
  const int64_t S = S_, rows = (S * M + 1) / 2 * 2;
  ConstrainedBlock b{};
  b.viol = 0;
  b.vals = b.viol + rows;
  b.pts = b.vals + (values ? rows : 0);
  b.f = b.pts + (int64_t)GPBO_MAX_PATHS * DP;
  b.doubles = b.f + S * GPBO_MAX_PATHS;
  return b;
}

}  // namespace gpbo
