// gpbo_sample_paths (gfx950): S <= 16 function draws from the slot's posterior, evaluated over the resident candidates, and each
// draw's maximiser — Thompson sampling by pathwise conditioning (Matheron's rule; Wilson et al. 2020).
//
// Replaces GaussianProcessRegressor.sample_y (_gpr.py: predict(return_cov=True) + an M x M factorisation on the host), which stops
// at the M <= 16384 of gpbo_predict_cov.  A draw is
//   f_s(x) = g_s(x) + sum_i k(x, X_i) v_s,i,     v_s = (K + eta I)^-1 (y_n - g_s(X) - eps_s) = alpha - W^T (W (g_s(X) + eps_s)),
// g_s(x) = fs sum_j weights[s, j] cos(2 pi (omega_j . xs + phase_j)) a random-Fourier-feature draw from the prior.  The rule is exact
// in the data; only the prior part is approximate.  Per candidate that is ONE k* generation and ONE feature generation — O((N + F) d)
// — contracted with S weight vectors each, against the O(N^2) of a posterior pass.
//
// Three kernels:
//   path_eval_kernel   the hot path, a sibling of posterior_refresh_kernel: thread = point with its coordinates in registers; the
//                      train points (phase 1), then the features (phase 2) staged through LDS 64 at a time and read back as
//                      broadcasts; one fma per path and element.  Run twice per call: over the train points with no phase 1
//                      (g_s(X), so that the prior draw at the data is the arithmetic the candidates get), then over the candidates.
//   path_t_kernel      T = W (g(X) + eps): a wave per (row, path), the lower triangle of W only.
//   path_v_kernel      V = alpha - W^T T: a thread per (column, path), four row groups per workgroup.
// The two small ones are 2 N^2 S flops each and not the hot path.  Every sum has a fixed order and no path's arithmetic depends on
// how many paths run beside it: path s alone and path s among 16 give the same bits.  fp64 whatever the slot's precision.
//
// gpbo_sample_paths_constrained runs path_eval_kernel once per slot with another EPILOGUE behind the same accumulators (path_plan.h:
// PathEpilogue): a constraint slot folds its S violation terms per candidate into a resident viol[S][M], the objective reads viol and
// stores the selection key.  The values themselves are the ones gpbo_sample_paths stores, bit for bit.
#include "gpbo_internal.h"

namespace gpbo {

constexpr int PT_CH = 64;           // train points / features per LDS stage

struct PathEvalArgs {
  const double* Xs;       // [NP][DP] scaled train points
  const double* V;        // [S][NP] path weights, zero from row N on
  const double* P;        // [>= M][DP] the scaled points the paths are evaluated at
  const double* omega;    // (F, d) turns per unit of the scaled input
  const double* phase;    // (F,) turns
  const double* weights;  // (S, F)
  double* out;            // [S][ld]: y_std * f + y_mean, negated when `negate` (the selection key)
  int64_t M, ld;
  int N, NP, F, d, S;     // N = 0: no phase 1 (the prior draw alone)
  int negate;
  double fs, y_mean, y_std;
  // gpbo_sample_paths_constrained (path_plan.h: PathEpilogue; PATH_PLAIN reads none of these)
  int epilogue;
  double lb, ub;          // a constraint slot's bounds
  double* viol;           // [S][ld] the violations: written / added to by a constraint slot, read by the objective
  double* vals;           // [S][ld] the values themselves, or null
};

// NS = accumulators held per point (paths c >= S are zero columns: they add nothing and are not written), indexed by unrolled
// loops only, so they stay registers.
template <int DP, int KERNEL, int NS>
__global__ __launch_bounds__(256) void path_eval_kernel(const PathEvalArgs a) {
  __shared__ __attribute__((aligned(16))) double xs[PT_CH * DP];     // phase 1: train points; phase 2: omega [feature][DP]
  __shared__ __attribute__((aligned(16))) double wt[PT_CH * NS];     // [train point | feature][path]
  __shared__ double ph[PT_CH];
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = m < a.M;
  double xc[DP];
  {
    const double* xcp = a.P + (live ? m : 0) * DP;
#pragma unroll
    for (int t = 0; t < DP; t += 2) {
      const double2 v = *reinterpret_cast<const double2*>(xcp + t);
      xc[t] = v.x;
      xc[t + 1] = v.y;
    }
  }
  double acc[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) acc[c] = 0.0;
  // phase 1: sum_i k(x, X_i) v_s,i
  const int k_end = (a.N + PT_CH - 1) / PT_CH * PT_CH;      // <= NP: NP is a multiple of 64
  for (int kc = 0; kc < k_end; kc += PT_CH) {
    __syncthreads();
    {
      const double2* src = reinterpret_cast<const double2*>(a.Xs + (int64_t)kc * DP);
      double2* dst = reinterpret_cast<double2*>(xs);
      for (int e = threadIdx.x; e < PT_CH * DP / 2; e += blockDim.x) dst[e] = src[e];
      for (int e = threadIdx.x; e < PT_CH * NS; e += blockDim.x) {
        const int c = e / PT_CH, kk = e - c * PT_CH;      // consecutive threads = consecutive entries of one path's weights
        const int i = kc + kk;
        wt[kk * NS + c] = (c < a.S && i < a.N) ? a.V[(int64_t)c * a.NP + i] : 0.0;
      }
    }
    __syncthreads();
    if (!live) continue;
#pragma unroll 2
    for (int kk = 0; kk < PT_CH; kk += 2) {
      const double* xr = xs + kk * DP;           // the same address in every lane: LDS broadcast
      double d2a = 0.0, d2b = 0.0;
#pragma unroll
      for (int t = 0; t < DP; ++t) {
        const double da = xc[t] - xr[t], db = xc[t] - xr[DP + t];
        d2a = fma(da, da, d2a);
        d2b = fma(db, db, d2b);
      }
      const double ka = gpbo_kernel_value<KERNEL>(d2a);
      const double kb = gpbo_kernel_value<KERNEL>(d2b);
      const double* wa = wt + kk * NS;
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        acc[c] = fma(ka, wa[c], acc[c]);
        acc[c] = fma(kb, wa[NS + c], acc[c]);
      }
    }
  }
  // phase 2: + sum_j (fs weights[s, j]) cos(2 pi (omega_j . xs + phase_j)).  The argument is in turns, so its reduction
  // r = t - rint(t) is exact whatever the frequency; a padded feature has weight 0.
  for (int jc = 0; jc < a.F; jc += PT_CH) {
    __syncthreads();
    for (int e = threadIdx.x; e < PT_CH * DP; e += blockDim.x) {
      const int j = e / DP, t = e - j * DP;
      xs[e] = (jc + j < a.F && t < a.d) ? a.omega[(int64_t)(jc + j) * a.d + t] : 0.0;
    }
    for (int e = threadIdx.x; e < PT_CH; e += blockDim.x) ph[e] = (jc + e < a.F) ? a.phase[jc + e] : 0.0;
    for (int e = threadIdx.x; e < PT_CH * NS; e += blockDim.x) {
      const int c = e / PT_CH, kk = e - c * PT_CH;
      wt[kk * NS + c] = (c < a.S && jc + kk < a.F) ? a.fs * a.weights[(int64_t)c * a.F + jc + kk] : 0.0;
    }
    __syncthreads();
    if (!live) continue;
#pragma unroll 2
    for (int kk = 0; kk < PT_CH; ++kk) {
      const double* om = xs + kk * DP;
      double t = ph[kk];
#pragma unroll
      for (int k = 0; k < DP; ++k) t = fma(om[k], xc[k], t);
      const double r = t - __builtin_rint(t);      // |r| <= 1/2
      const double cv = cospi(r + r);
      const double* wa = wt + kk * NS;
#pragma unroll
      for (int c = 0; c < NS; ++c) acc[c] = fma(cv, wa[c], acc[c]);
    }
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < NS; ++c) {
    if (c < a.S) {
      const double f = fma(a.y_std, acc[c], a.y_mean);
      const int64_t at = (int64_t)c * a.ld + m;
      if (a.epilogue == PATH_PLAIN) {
        a.out[at] = a.negate ? -f : f;
        continue;
      }
      if (a.vals) a.vals[at] = f;
      if (a.epilogue == PATH_KEY) {
        // the selection takes the first NaN, else the least key: -f where the constraint draws call the point feasible, +inf elsewhere
        const double v = a.viol[at];
        a.out[at] = (f != f || v != v) ? __builtin_nan("") : (v == 0.0 ? -f : __builtin_inf());
      } else if (a.epilogue == PATH_MASKED) {
        // the value a greedy step scores (gpbo_cnei_greedy): f itself where the point is feasible, -inf elsewhere
        const double v = a.viol[at];
        a.out[at] = (f != f || v != v) ? __builtin_nan("") : (v == 0.0 ? f : -__builtin_inf());
      } else {
        // t = max(max(lb - c, c - ub), 0) / y_std, a NaN c kept (fmax would drop it)
        const double g = fmax(a.lb - f, f - a.ub);
        const double t = (f != f) ? f : fmax(g, 0.0) / a.y_std;
        a.viol[at] = a.epilogue == PATH_VIOL_WRITE ? t : a.viol[at] + t;
      }
    }
  }
}

// T[s][r] = sum_{i <= r} W[r, i] (G[s][i] + eps[s][i]) for r < N, 0 for N <= r < NP.  A wave per (row, path): lane l takes the
// columns l, l + 64, ... in order, the 64 partial sums are added by a butterfly (every lane ends with the same value).
__global__ __launch_bounds__(256) void path_t_kernel(const double* __restrict__ W, const double* __restrict__ G,
                                                     const double* __restrict__ eps, double* __restrict__ T, int N, int NP) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int s = blockIdx.y;
  if (r >= NP) return;
  double acc = 0.0;
  if (r < N) {
    const double* wr = W + (int64_t)r * NP;
    const double* g = G + (int64_t)s * NP;
    const double* e = eps + (int64_t)s * N;
    for (int i = lane; i <= r; i += 64) acc = fma(wr[i], g[i] + e[i], acc);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) T[(int64_t)s * NP + r] = acc;
}

// V[s][i] = alpha[i] - sum_{i <= r < N} W[r, i] T[s][r] for i < N, 0 for N <= i < NP.  Thread = column i (consecutive lanes read
// consecutive entries of a row of W); the rows of a column go to four groups, r = first row of the tile + g, + 4, ..., whose sums
// are added as (g0 + g1) + (g2 + g3).
__global__ __launch_bounds__(256) void path_v_kernel(const double* __restrict__ W, const double* __restrict__ T,
                                                     const double* __restrict__ alpha, double* __restrict__ V, int N, int NP) {
  __shared__ double sh[4][64];
  const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 64 + lane;
  const int s = blockIdx.y;
  const double* t = T + (int64_t)s * NP;
  double acc = 0.0;
  for (int r = blockIdx.x * 64 + g; r < N; r += 4)
    if (r >= i) acc = fma(W[(int64_t)r * NP + i], t[r], acc);
  sh[g][lane] = acc;
  __syncthreads();
  if (g == 0) {
    const double sum = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
    V[(int64_t)s * NP + i] = i < N ? alpha[i] - sum : 0.0;
  }
}

template <int NS>
static int launch_path_eval_ns(gpbo_ctx* ctx, const Model& m, const PathEvalArgs& a) {
  const unsigned threads = path_eval_threads(a.M);
  const int64_t blocks = (a.M + threads - 1) / threads;
  if (blocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "sample_paths: grid too large; shard the candidates");
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    path_eval_kernel<decltype(dp)::value, decltype(k)::value, NS><<<dim3((unsigned)blocks), dim3(threads), 0, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

static int launch_path_eval(gpbo_ctx* ctx, const Model& m, const PathEvalArgs& a) {
  switch (path_eval_ns(a.S)) {
    case 1: return launch_path_eval_ns<1>(ctx, m, a);
    case 4: return launch_path_eval_ns<4>(ctx, m, a);
    default: return launch_path_eval_ns<GPBO_MAX_PATHS>(ctx, m, a);
  }
}

static PathEvalArgs path_eval_args(const Model& m, const PathWorkspace& ws, int S, int F) {
  PathEvalArgs a{};
  a.Xs = m.Xs; a.V = ws.p(ws.at.V); a.omega = ws.p(ws.at.omega); a.phase = ws.p(ws.at.phase); a.weights = ws.p(ws.at.weights);
  a.NP = (int)m.NP; a.F = F; a.d = m.d; a.S = S;
  a.fs = path_feature_scale(m.amplitude, F);
  return a;
}

// V[s] = a - W^T (W (G[s] + eps[s])) for S columns: G, T, V [S][NP], eps [S][N], a [NP] (the slot's alpha; kg.hip passes zeros for
// eps and a and gets -K'^-1 G[s]).  Each column's arithmetic is its own: S columns or one give the same bits.
int launch_path_solve(gpbo_ctx* ctx, const Model& m, int S, const double* G, const double* eps, const double* a, double* T, double* V) {
  const int N = (int)m.N, NP = (int)m.NP;
  path_t_kernel<<<dim3((unsigned)((NP + 3) / 4), (unsigned)S), dim3(256), 0, ctx->stream>>>(m.W, G, eps, T, N, NP);
  GPBO_HIP(ctx, hipGetLastError());
  path_v_kernel<<<dim3((unsigned)(NP / 64), (unsigned)S), dim3(256), 0, ctx->stream>>>(m.W, T, a, V, N, NP);
  GPBO_HIP(ctx, hipGetLastError());
  return GPBO_OK;
}

// The draws' inputs made resident and V = alpha - W^T (W (g(X) + eps)) of the S paths: everything a path's value (path_eval_kernel)
// or its ascent (path_ascent.hip) reads, in the context's paths workspace (path_plan.h), with room for n_runs ascent runs behind it.
int launch_path_weights(gpbo_ctx* ctx, const Model& m, int S, int F, const double* omega, const double* phase, const double* weights,
                        const double* eps, int n_runs, PathWorkspace* ws) {
  const int N = (int)m.N, NP = (int)m.NP;
  int rc;
  const PathBlock b = path_block(S, F, N, NP, m.d, n_runs);
  if ((rc = ensure(ctx, &ctx->paths, &ctx->cap_paths, b.doubles))) return rc;
  *ws = {ctx->paths, b};
  double *eps_d = ws->p(b.eps), *G = ws->p(b.G), *T = ws->p(b.T);
  GPBO_HIP(ctx, hipMemcpyAsync(ws->p(b.omega), omega, (size_t)(b.phase - b.omega) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(ws->p(b.phase), phase, (size_t)F * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(ws->p(b.weights), weights, (size_t)(b.eps - b.weights) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(eps_d, eps, (size_t)(b.G - b.eps) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  // g_s(X): the prior draws at the train points, by the kernel the candidates get
  PathEvalArgs a = path_eval_args(m, *ws, S, F);
  a.P = m.Xs; a.out = G; a.M = N; a.ld = NP; a.N = 0; a.negate = 0; a.y_mean = 0.0; a.y_std = 1.0;
  if ((rc = launch_path_eval(ctx, m, a))) return rc;
  return launch_path_solve(ctx, m, S, G, eps_d, m.alpha, T, ws->p(b.V));
}

// The S paths of gpbo_sample_paths over the M resident candidates: the negated values land in ctx->ys as S rows of M (the
// selection's keys), nothing of the slot or the candidates is written.  The caller has checked every argument.  n_runs / ws: as
// launch_path_weights (gpbo_ascend_paths goes on from the same workspace).
// `fold` (null: gpbo_sample_paths): the slot's part of gpbo_sample_paths_constrained instead of the plain store
static int sample_paths_over_candidates(gpbo_ctx* ctx, const Model& m, int64_t M, double y_mean, double y_std, int S, int F,
                                        const double* omega, const double* phase, const double* weights, const double* eps, int n_runs,
                                        PathWorkspace* ws_out, const PathFold* fold) {
  int rc;
  if ((rc = launch_path_weights(ctx, m, S, F, omega, phase, weights, eps, n_runs, ws_out))) return rc;
  const PathWorkspace& ws = *ws_out;
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * m.DP))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, m.d, m.DP, m.ls, ctx->Xcs, Mp))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, (int64_t)S * M))) return rc;
  // the paths over the candidates
  PathEvalArgs a = path_eval_args(m, ws, S, F);
  a.P = ctx->Xcs; a.out = ctx->ys; a.M = M; a.ld = M; a.N = (int)m.N; a.negate = 1; a.y_mean = y_mean; a.y_std = y_std;
  if (fold) { a.epilogue = fold->epilogue; a.lb = fold->lb; a.ub = fold->ub; a.viol = fold->viol; a.vals = fold->vals; }
  return launch_path_eval(ctx, m, a);
}

int launch_sample_paths(gpbo_ctx* ctx, const Model& m, int64_t M, double y_mean, double y_std, int S, int F, const double* omega,
                        const double* phase, const double* weights, const double* eps, int n_runs, PathWorkspace* ws_out) {
  return sample_paths_over_candidates(ctx, m, M, y_mean, y_std, S, F, omega, phase, weights, eps, n_runs, ws_out, nullptr);
}

// One slot's pass of gpbo_sample_paths_constrained: the slot's S draws over the M resident candidates, and behind the accumulators
// what fold->epilogue says (path_plan.h) — a constraint slot's violation terms into fold->viol, the objective's selection keys into
// ctx->ys.  Nothing but ctx->ys, ctx->Xcs, the two workspaces is written.
int launch_sample_paths_fold(gpbo_ctx* ctx, const Model& m, int64_t M, double y_mean, double y_std, int S, int F, const double* omega,
                             const double* phase, const double* weights, const double* eps, const PathFold& fold, PathWorkspace* ws) {
  return sample_paths_over_candidates(ctx, m, M, y_mean, y_std, S, F, omega, phase, weights, eps, 0, ws, &fold);
}

// f[s * ld + r] = path s of the workspace's draws (those of the last pass, the model m's) at the scaled candidate idx[r], r < n <= 16,
// by the kernel instance and the arithmetic the pass itself ran: the bits the pass had for that candidate.  pts: n * DP doubles.
int launch_paths_at(gpbo_ctx* ctx, const Model& m, const PathWorkspace& ws, double y_mean, double y_std, int S, int F,
                    const int64_t* idx, int n, double* pts, double* f, int ld) {
  for (int r = 0; r < n; ++r)
    GPBO_HIP(ctx, hipMemcpyAsync(pts + (int64_t)r * m.DP, ctx->Xcs + idx[r] * m.DP, (size_t)m.DP * sizeof(double),
                                 hipMemcpyDeviceToDevice, ctx->stream));
  return launch_paths_over(ctx, m, ws, y_mean, y_std, S, F, pts, n, f, ld);
}

// f[s * ld + r] = path s of the workspace's draws at the scaled point P_r, r < n: path_eval_kernel with both phases and the plain
// store — over the scaled candidates with ld = M these are the values gpbo_sample_paths has, before their negation.
int launch_paths_over(gpbo_ctx* ctx, const Model& m, const PathWorkspace& ws, double y_mean, double y_std, int S, int F,
                      const double* P, int64_t n, double* f, int64_t ld) {
  PathEvalArgs a = path_eval_args(m, ws, S, F);
  a.P = P; a.out = f; a.M = n; a.ld = ld; a.N = (int)m.N; a.negate = 0; a.y_mean = y_mean; a.y_std = y_std;
  return launch_path_eval(ctx, m, a);
}

// ... with an epilogue behind the accumulators (path_plan.h: PathEpilogue) instead of the plain store: a constraint slot's terms
// into fold.viol [S][ld] (f is not written and may be null), the objective's key or masked value into f.  fold.viol and fold.vals
// have f's leading dimension.  The values are launch_paths_over's, bit for bit.
int launch_paths_over_fold(gpbo_ctx* ctx, const Model& m, const PathWorkspace& ws, double y_mean, double y_std, int S, int F,
                           const double* P, int64_t n, double* f, int64_t ld, const PathFold& fold) {
  PathEvalArgs a = path_eval_args(m, ws, S, F);
  a.P = P; a.out = f; a.M = n; a.ld = ld; a.N = (int)m.N; a.negate = 0; a.y_mean = y_mean; a.y_std = y_std;
  a.epilogue = fold.epilogue; a.lb = fold.lb; a.ub = fold.ub; a.viol = fold.viol; a.vals = fold.vals;
  return launch_path_eval(ctx, m, a);
}

}  // namespace gpbo
