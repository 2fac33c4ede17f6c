// gpbo_ascend_paths (gfx950): each posterior function draw of gpbo_sample_paths climbed from its starts to a local maximiser inside
// the box, one workgroup per run (path s, start k), evaluations AND optimiser in ONE launch (Wilson et al. 2020 maximise their
// pathwise-conditioned draws by gradient ascent: a draw is a closed-form function, its gradient costs what its value costs).
//
//   f_s(x)      = y_std (fs sum_j w_sj cos(2 pi t_j) + sum_i v_si k(xs, Xs_i)) + y_mean,   xs = x / l,  t_j = omega_j . xs + phase_j
//   df_s / dx_t = y_std (-2 pi fs sum_j w_sj sin(2 pi t_j) omega_jt + sum_i v_si slope(|xs - Xs_i|^2) (xs_t - Xs_it)) / l_t
// with slope = gpbo_kernel_slope<KERNEL> (gpbo_internal.h: dk / dxs_t = slope * (xs_t - Xs_t); nu = 0.5 gives 0 ON a training point).
// No W walk, no variance term, no size limit: O((N + F) d) per evaluation against the O(N^2) of polish_rows_kernel.
//
// path_ascend_kernel<DP, KERNEL>, 256 threads:
//   * thread t takes the training points t, t + 256, ... and then the features t, t + 256, ..., with 1 + DP partial sums (value |
//     gradient in the scaled input) in registers; the trial point is read from LDS as a broadcast;
//   * the partial sums are added inside the rows of 16 lanes by four DPP steps (no LDS traffic), the 16 rows' totals cross through
//     LDS and wave 0, lane = variable, adds them row 0 ... 15: every sum has one fixed order, whatever else is in the grid;
//   * wave 0 then takes the optimiser's step on -f_s (polish_lane_opt.h: pr_advance, the code of polish_rows_kernel) and leaves the
//     next trial point in LDS.  Two barriers per evaluation.
// The feature argument stays in turns (r = t - rint(t), cospi / sinpi of 2 r), as path_eval_kernel reduces it.  fp64 whatever the
// slot's precision.  The trial points live in the kernel: the candidate buffer is read (the starts), never written.
#include "gpbo_internal.h"
#include "polish_lane_opt.h"

namespace gpbo {

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_ROWS = PA_THREADS / 16;      // DPP rows of 16 lanes in a workgroup

struct PathAscentArgs {
  const double *Xs, *V;                 // [NP][DP] scaled train points; [S][NP] path weights
  const double *omega, *phase, *weights, *ls;      // (F, d), (F,), (S, F), (d,)
  const double* starts;                 // (S K, d), or null: the rows start_idx of Xc
  const int64_t* start_idx;             // (S K)
  const double* Xc;                     // [M][d] the resident candidates
  int64_t M;
  const double *lo, *hi;                // (d,)
  double *x_out, *f_out, *g_out;        // (S K, d), (S K), (S K, d)
  int *status_out, *eval_out;           // (S K)
  int N, NP, F, d, K, max_iter;         // max_iter = 0: the value and gradient at the (clipped) start, no search
  double fs, y_mean, y_std;
};

template <int DP, int KERNEL>
__global__ __launch_bounds__(PA_THREADS) void path_ascend_kernel(const PathAscentArgs a) {
  __shared__ double xs[DP];                              // the trial point, length-scaled
  __shared__ double red[PA_ROWS * (DP + 1)];             // [row of 16 lanes][value | gradient]
  __shared__ double opt[2 * LBFGS_M * DP + 4 * LBFGS_M]; // the optimiser's block (search_plan.h: polish_opt_doubles(d), d <= DP)
  __shared__ int flag;
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int run_idx = (int)blockIdx.x, s = run_idx / a.K;
  const int d = a.d;
  const bool mine = lane < d;

  RowsRun run{};
  double ls_t = 1.0;      // this lane's length scale
  if (wave == 0) {
    run.lo = mine ? a.lo[lane] : 0.0;
    run.hi = mine ? a.hi[lane] : 0.0;
    double x0 = 0.0;
    if (mine) {
      if (a.starts) {
        x0 = a.starts[(int64_t)run_idx * d + lane];
      } else {
        const int64_t r = a.start_idx[run_idx];
        x0 = (r >= 0 && r < a.M) ? a.Xc[r * d + lane] : __builtin_nan("");
      }
      ls_t = a.ls[lane];
    }
    run.xt = mine ? polish_min(polish_max(x0, run.lo), run.hi) : 0.0;      // polish_start
    run.alpha = 1.0;
    run.status = 2;
    if (lane < DP) xs[lane] = mine ? run.xt / ls_t : 0.0;
    if (lane == 0) flag = 0;
  }
  __syncthreads();

  const double* __restrict__ Vs = a.V + (int64_t)s * a.NP;
  const double* __restrict__ ws = a.weights + (int64_t)s * a.F;
  const int round_cap = 4 * a.max_iter + 64;

  for (int round = 0;; ++round) {
    double acc[DP + 1];      // [0] the value, [1 + t] the gradient in the scaled input
#pragma unroll
    for (int c = 0; c <= DP; ++c) acc[c] = 0.0;
    // ---- the training points: sum_i v_si k(xs, Xs_i)
    for (int i = tid; i < a.N; i += PA_THREADS) {
      const double* __restrict__ xr = a.Xs + (int64_t)i * DP;
      double df[DP];
      double d2 = 0.0;
#pragma unroll
      for (int t = 0; t < DP; ++t) {
        df[t] = xs[t] - xr[t];
        d2 = fma(df[t], df[t], d2);
      }
      const double kv = gpbo_kernel_value<KERNEL>(d2);
      const double v = Vs[i];
      const double c = v * gpbo_kernel_slope<KERNEL>(d2, kv);
      acc[0] = fma(v, kv, acc[0]);
#pragma unroll
      for (int t = 0; t < DP; ++t) acc[1 + t] = fma(c, df[t], acc[1 + t]);
    }
    // ---- the features: fs sum_j w_sj cos(2 pi t_j); the argument in turns, so r = t - rint(t) is exact whatever the frequency
    for (int j = tid; j < a.F; j += PA_THREADS) {
      const double* __restrict__ orow = a.omega + (int64_t)j * d;
      double om[DP];
      double t = a.phase[j];
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        om[k] = (k < d) ? orow[k] : 0.0;
        t = fma(om[k], xs[k], t);
      }
      const double r = t - __builtin_rint(t);      // |r| <= 1/2
      const double w = a.fs * ws[j];
      acc[0] = fma(w, cospi(r + r), acc[0]);
      const double c = (-6.28318530717958647693 * w) * sinpi(r + r);
#pragma unroll
      for (int k = 0; k < DP; ++k) acc[1 + k] = fma(c, om[k], acc[1 + k]);
    }
    // ---- the rows of 16 lanes (DPP, as pr_sum's steps), then the rows' totals through LDS
    {
      const int row = tid >> 4, r16 = tid & 15;
#pragma unroll
      for (int c = 0; c <= DP; ++c) {
        double v = acc[c];
        v += pr_dpp<0xB1>(v);
        v += pr_dpp<0x4E>(v);
        v += pr_dpp<0x141>(v);
        v += pr_dpp<0x140>(v);
        if ((c & 15) == r16) red[row * (DP + 1) + c] = v;
      }
    }
    __syncthreads();
    // ---- wave 0, lane = variable: the rows in order, the objective -f_s and its gradient in x, the optimiser's step
    if (wave == 0) {
      double fsum = 0.0, gsum = 0.0;
      const int t = lane < DP ? lane : 0;
      for (int r = 0; r < PA_ROWS; ++r) {
        fsum += red[r * (DP + 1)];
        gsum += red[r * (DP + 1) + 1 + t];
      }
      const double ft = -fma(a.y_std, fsum, a.y_mean);
      double gt = 0.0;
      if (mine) {
        gt = -((a.y_std * gsum) / ls_t);
        if (!__builtin_isfinite(gt)) gt = 0.0;
      }
      if (a.max_iter == 0) {
        run.x = run.xt; run.g = gt; run.f = ft;
        run.evals = 1;
        run.phase = 2;
        run.status = (__builtin_isfinite(ft) &&
                      pr_max_abs(polish_min(polish_max(run.x - run.g, run.lo), run.hi) - run.x, d) <= POLISH_PGTOL) ? 0 : 2;
        if (lane == 0) flag = 1;
      } else {
        pr_advance(run, ft, gt, d, lane, opt, a.max_iter);
        if (lane < DP) xs[lane] = mine ? run.xt / ls_t : 0.0;
        if (lane == 0) flag = (run.phase == 2 || round + 1 > round_cap) ? 1 : 0;
      }
    }
    __syncthreads();
    if (flag) break;
  }
  if (wave == 0) {
    if (mine) {
      a.x_out[(int64_t)run_idx * d + lane] = run.x;
      a.g_out[(int64_t)run_idx * d + lane] = -run.g;
    }
    if (lane == 0) {
      a.f_out[run_idx] = -run.f;
      a.status_out[run_idx] = run.phase == 2 ? run.status : 2;
      a.eval_out[run_idx] = run.evals;
    }
  }
}

}  // namespace

// The runs of gpbo_ascend_paths over the path weights `ws` left by launch_path_weights / launch_sample_paths, laid out for S K runs
// (path_plan.h).  starts (S K, d) on the host, or null: the rows start_idx (S K, local indices, host) of the
// resident candidates.  Synchronises; the results land in the caller's arrays (g_out / eval_out may be null).
int launch_path_ascent(gpbo_ctx* ctx, const Model& m, const PathWorkspace& ws, int S, int K, int F, double y_mean, double y_std,
                       const double* starts, const int64_t* start_idx, const double* box_lo, const double* box_hi, int max_iter,
                       double* x_out, double* f_out, double* g_out, int* status_out, int* eval_out) {
  const int d = m.d, R = S * K;
  const int64_t n_x = (int64_t)R * d;
  const PathBlock& b = ws.at;
  double *lo_d = ws.p(b.lo), *hi_d = ws.p(b.hi), *st_d = ws.p(b.starts), *x_d = ws.p(b.x), *g_d = ws.p(b.g), *f_d = ws.p(b.f);
  int64_t* idx_d = reinterpret_cast<int64_t*>(ws.p(b.start_idx));
  int* status_d = reinterpret_cast<int*>(ws.base) + b.status;
  int* eval_d = reinterpret_cast<int*>(ws.base) + b.evals;
  GPBO_HIP(ctx, hipMemcpyAsync(lo_d, box_lo, (size_t)d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(hi_d, box_hi, (size_t)d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (starts) GPBO_HIP(ctx, hipMemcpyAsync(st_d, starts, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  else GPBO_HIP(ctx, hipMemcpyAsync(idx_d, start_idx, (size_t)R * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  PathAscentArgs a{};
  a.Xs = m.Xs; a.V = ws.p(b.V); a.omega = ws.p(b.omega); a.phase = ws.p(b.phase); a.weights = ws.p(b.weights); a.ls = m.ls;
  a.starts = starts ? st_d : nullptr; a.start_idx = idx_d; a.Xc = ctx->Xc; a.M = starts ? 0 : ctx->M;
  a.lo = lo_d; a.hi = hi_d;
  a.x_out = x_d; a.f_out = f_d; a.g_out = g_d; a.status_out = status_d; a.eval_out = eval_d;
  a.N = (int)m.N; a.NP = (int)m.NP; a.F = F; a.d = d; a.K = K; a.max_iter = max_iter;
  a.fs = path_feature_scale(m.amplitude, F);
  a.y_mean = y_mean; a.y_std = y_std;
  if (const int rc = with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
        path_ascend_kernel<decltype(dp)::value, decltype(k)::value><<<dim3((unsigned)R), dim3(PA_THREADS), 0, ctx->stream>>>(a);
        GPBO_HIP(ctx, hipGetLastError());
        return GPBO_OK;
      }))
    return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(x_out, x_d, (size_t)n_x * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(f_out, f_d, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (g_out) GPBO_HIP(ctx, hipMemcpyAsync(g_out, g_d, (size_t)n_x * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(status_out, status_d, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (eval_out) GPBO_HIP(ctx, hipMemcpyAsync(eval_out, eval_d, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GPBO_OK;
}

}  // namespace gpbo
