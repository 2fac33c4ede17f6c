// Integrated posterior variance reduction (Cohn's ALC; IMSE-optimal design; qNegIntegratedPosteriorVariance at q = 1) over the
// resident candidates (gfx950): gpiv_ivr_argbest's values.  include/gpiv.h has the formulas and the conventions; ivr_plan.h the
// dispatch rule, the packing of V and the workspace.  Per candidate x and integration point a_j:
//   cov_j(x) = c (k(x, a_j) + sum_i k(x, X_i) V_j,i),      V_j = -W^T (W k*(a_j)) = -K'^-1 k*(a_j)
//   ys[x]    = -(y_std^2 (sum_j omega_j cov_j(x)^2) / ((v + lambda) - w))
// an (M x N) (N x J) product with a squared, weighted row sum behind it.  The M x J block never exists: not in memory, not in LDS.
// Compiled with -ffp-contract=off, as kg.hip (the fmas below are written out).
//
// Three stages:
//   points   per group of IVR_GROUP columns: ivr_points_kernel (k*(a_j) over the train points), launch_path_solve (posterior_paths.hip)
//            with zero noise draws and a zero vector for alpha leaves V_j, ivr_pack_kernel scatters it into the fragment-packed
//            image.  2 N^2 J flops on GEMV kernels: not the hot path.
//   score    ivr_score_kernel, the hot path.  A workgroup of four waves owns 64 candidates.  Thread (wave w, lane l) keeps
//            candidate l's scaled coordinates in registers for the whole kernel.  Per stage of IVR_KC = 32 train points the
//            points' rows go through LDS and come back as broadcasts; wave w generates k(x_l, X_i) for the 8 points 8 w .. 8 w + 7
//            of the stage into a k-major LDS block [32][68]: the A operand.  Every wave then multiplies the whole block into ITS
//            16 NSUB columns of the tile, 8 k-steps x 4 row fragments x NSUB column fragments of v_mfma_f64_16x16x4_f64, the
//            accumulators 64 x 16 NSUB fp64 per wave (128 registers at NSUB = 4).  The B fragments come straight from the packed V
//            (L2 / HBM -> registers, one 512-byte line per load), requested before the stage's generation and used after it.  One
//            kernel value feeds 128 NSUB matrix flops.  J > 256 walks the tiles inside the kernel and regenerates k* per tile.
//            Behind a tile's last stage its own points take the same route once more: wave w generates k(x_l, a_j) for ITS columns,
//            8 at a time, and the matrix core adds them through a unit B fragment (1.0 where the k index is the column) — one
//            rounding, the sum's last term.  Then c, the square and omega_j in registers, the NSUB fragments in order, the 16
//            columns of a fragment by a butterfly (xor 1, 2, 4, 8), the four waves in wave order through LDS, the tiles in tile
//            order into the candidate's running sum.  After the last tile y_std^2 / den^2 and the conventions, and ctx->ys.
//   select   the existing arg-best / top-k over ctx->ys (acq_kernels.hip), from the entry point.
// A candidate's bits depend neither on M nor on the other candidates: a row of the product reads its own row of A only, and every
// sum above has a fixed order.  Rows from M on repeat row M - 1 and are not written.
#include "gpbo_internal.h"
#include "ivr_plan.h"
#include "ivr_product.h"

#include <cmath>

namespace gpbo {

// KS[j][i] = k(a_j, X_i) for i < N, 0 up to NP.  Workgroup = point; thread t takes the train points t, t + 256, ...
template <int DP, int KERNEL>
__global__ __launch_bounds__(256) void ivr_points_kernel(const double* __restrict__ Xs, const double* __restrict__ As,
                                                         double* __restrict__ KS, int N, int NP) {
  const int j = blockIdx.x;
  double xa[DP];
#pragma unroll
  for (int t = 0; t < DP; ++t) xa[t] = As[(int64_t)j * DP + t];
  for (int i = threadIdx.x; i < NP; i += 256) {
    double kv = 0.0;
    if (i < N) {
      const double* xr = Xs + (int64_t)i * DP;
      double d2 = 0.0;
#pragma unroll
      for (int t = 0; t < DP; ++t) {
        const double df = xa[t] - xr[t];
        d2 = fma(df, df, d2);
      }
      kv = gpbo_kernel_value<KERNEL>(d2);
    }
    KS[(int64_t)j * NP + i] = kv;
  }
}

// omega[j] = the caller's weight, or `uniform` without one, for j < J; 0 up to Jp
__global__ void ivr_omega_kernel(const double* __restrict__ wraw, int has_weights, double uniform, int J, int Jp,
                                 double* __restrict__ omega) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Jp) return;
  omega[j] = j < J ? (has_weights ? wraw[j] : uniform) : 0.0;
}

// The group's columns [j0, j0 + cols) of V [.][NP] into the packed image (ivr_plan.h); a column from J on and a row from N on are 0.
__global__ void ivr_pack_kernel(const double* __restrict__ V, double* __restrict__ Vp, int j0, int cols, int J, int N, int NP, int Kp,
                                int nsub) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)cols * Kp) return;
  const int jl = (int)(e / Kp), i = (int)(e - (int64_t)jl * Kp);
  const int j = j0 + jl;
  const double v = (j < J && i < N) ? V[(int64_t)jl * NP + i] : 0.0;
  Vp[ivr_packed_index(i, j, nsub, Kp)] = v;
}

struct IvrScoreArgs {
  const double* Xs;       // [NP][DP] scaled train points
  const double* Vp;       // fragment-packed V (ivr_plan.h), Jp x Kp doubles
  const double* P;        // [>= M][DP] the scaled candidates
  const double* As;       // [Jp][DP] the scaled points, zero rows from J on
  const double* omega;    // [Jp], zero from J on
  const double* mu;
  const double* sd;
  double* ys;
  int64_t M;
  int Kp, n_tiles;
  double amplitude, y_std, lambda, white;
};

template <int DP, int KERNEL, int NSUB>
__global__ __launch_bounds__(256) void ivr_score_kernel(const IvrScoreArgs a) {
  __shared__ __attribute__((aligned(16))) double xs[IVR_KC * DP];           // the stage's train points (or the tile's own points)
  __shared__ __attribute__((aligned(16))) double ab[IVR_KC * IVR_PITCH];    // k* of the stage, k-major: the A operand
  __shared__ double red[4][IVR_ROWS];
  constexpr int NWC = 16 * NSUB;          // columns per wave
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lk = lane >> 4, lc = lane & 15;
  const int64_t m0 = (int64_t)blockIdx.x * IVR_ROWS;
  double xc[DP];
  ivr_load_candidate<DP>(a.P, m0, a.M, lane, xc);
  double total = 0.0;      // threads 0 .. 63: candidate tid's sum over the tiles so far
  for (int tile = 0; tile < a.n_tiles; ++tile) {
    iv_d4 acc[4][NSUB];
    ivr_tile_product<DP, KERNEL, NSUB>(a.Xs, a.Vp, a.As, a.Kp, tile, xc, xs, ab, acc);      // ivr_product.h
    const int64_t j0 = (int64_t)tile * (4 * NWC);
    // c, square, omega; the wave's columns; the four waves; the tiles
    double om[NSUB];
#pragma unroll
    for (int u = 0; u < NSUB; ++u) om[u] = a.omega[j0 + wave * NWC + 16 * u + lc];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < NSUB; ++u) {
          const double cov = a.amplitude * acc[t][u][r];
          s = s + om[u] * (cov * cov);
        }
#pragma unroll
        for (int off = 1; off <= 8; off <<= 1) s = s + __shfl_xor(s, off);
        if (lc == 0) red[wave][16 * t + lk + 4 * r] = s;
      }
    }
    __syncthreads();
    if (tid < IVR_ROWS) total = total + (((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]);
    __syncthreads();      // red and xs are free for the next tile
  }
  if (tid >= IVR_ROWS || m0 + tid >= a.M) return;
  const int64_t i = m0 + tid;
  const double mean = a.mu[i], sd = a.sd[i];
  if (mean != mean) { a.ys[i] = mean; return; }
  if (sd != sd) { a.ys[i] = sd; return; }
  const double q = sd / a.y_std;
  const double den2 = (q * q + a.lambda) - a.white;
  if (den2 == 0.0) { a.ys[i] = -0.0; return; }      // nothing is learned
  a.ys[i] = -(((a.y_std * a.y_std) * total) / den2);
}

// debug build: an event before and after each stage of the last call (gpiv_debug_stage_ms); the product records nothing
static inline void ivr_mark(gpbo_ctx* ctx, int i) {
#ifdef GPBO_DEBUG
  StageClock& c = ctx->iv_clock;
  if (!c.ev[i]) (void)hipEventCreate(&c.ev[i]);
  (void)hipEventRecord(c.ev[i], ctx->stream);
  c.used = (i == c.n - 1);
#else
  (void)ctx; (void)i;
#endif
}

template <int NSUB>
static int launch_ivr_score(gpbo_ctx* ctx, const Model& m, const IvrScoreArgs& a) {
  const int64_t blocks = (a.M + IVR_ROWS - 1) / IVR_ROWS;
  if (blocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "ivr_argbest: grid too large; shard the candidates");
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    ivr_score_kernel<decltype(dp)::value, decltype(k)::value, NSUB><<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

// The points stage into the workspace ws laid out by b: the scaled points, omega, and per group of columns k*(a_j), V_j and its packed
// image, event 0 of `clock` in front of the groups.  after_group (or null) runs behind each group's solve, while KS and V still
// hold that group's columns (sur.hip takes the points' means and variances there).
int launch_ivr_points(gpbo_ctx* ctx, const Model& m, double* ws, const IvrBlock& b, const double* points, const double* weights, int J,
                      StageClock& clock, IvrGroupHook after_group, void* user) {
  const int N = (int)m.N, NP = (int)m.NP, d = m.d, DP = m.DP;
  int rc;
  GPBO_HIP(ctx, hipMemcpyAsync(ws + b.raw, points, (size_t)J * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (weights) GPBO_HIP(ctx, hipMemcpyAsync(ws + b.wraw, weights, (size_t)J * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemsetAsync(ws + b.zero, 0, (size_t)b.n_zero * sizeof(double), ctx->stream));
  if ((rc = launch_prescale(ctx, ws + b.raw, J, d, DP, m.ls, ws + b.As, b.Jp))) return rc;
  ivr_omega_kernel<<<dim3((unsigned)((b.Jp + 255) / 256)), dim3(256), 0, ctx->stream>>>(ws + b.wraw, weights ? 1 : 0, 1.0 / (double)J, J,
                                                                                     (int)b.Jp, ws + b.omega);
  GPBO_HIP(ctx, hipGetLastError());
  // stage 1: k*(a_j), V_j, packed, a group of columns at a time
  jes_mark(ctx, clock, 0);
  for (int g0 = 0; g0 < J; g0 += IVR_GROUP) {
    const int cols = J - g0 < IVR_GROUP ? J - g0 : IVR_GROUP;
    rc = with_dp_kernel(ctx, DP, m.kernel, [&](auto dp, auto k) {
      ivr_points_kernel<decltype(dp)::value, decltype(k)::value><<<dim3((unsigned)cols), dim3(256), 0, ctx->stream>>>(
          m.Xs, ws + b.As + (int64_t)g0 * DP, ws + b.KS, N, NP);
      GPBO_HIP(ctx, hipGetLastError());
      return GPBO_OK;
    });
    if (rc) return rc;
    if ((rc = launch_path_solve(ctx, m, cols, ws + b.KS, ws + b.zero, ws + b.zero, ws + b.T, ws + b.V))) return rc;
    if (after_group && (rc = after_group(ctx, m, ws + b.KS, ws + b.V, g0, cols, user))) return rc;
    // the last group also writes the zero columns up to Jp
    const int pcols = g0 + cols == J ? (int)(b.Jp - g0) : cols;
    const int64_t n = (int64_t)pcols * b.Kp;
    ivr_pack_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(ws + b.V, ws + b.Vp, g0, pcols, J, N, NP,
                                                                                   (int)b.Kp, b.nsub);
    GPBO_HIP(ctx, hipGetLastError());
  }
  return GPBO_OK;
}

int launch_ivr_values(gpbo_ctx* ctx, const Model& m, int64_t M, const double* points, const double* weights, int J, double y_std) {
  const int d = m.d, DP = m.DP;
  int rc;
  const IvrBlock b = ivr_block(J, d, DP, m.N, m.NP);
  if ((rc = ensure(ctx, &ctx->iv, &ctx->cap_iv, b.doubles))) return rc;
  double* ws = ctx->iv;
  if ((rc = launch_ivr_points(ctx, m, ws, b, points, weights, J, ctx->iv_clock, nullptr, nullptr))) return rc;
  // stage 2: the scores
  ivr_mark(ctx, 1);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  IvrScoreArgs s{};
  s.Xs = m.Xs; s.Vp = ws + b.Vp; s.P = ctx->Xcs; s.As = ws + b.As; s.omega = ws + b.omega; s.mu = m.mu; s.sd = m.sd; s.ys = ctx->ys;
  s.M = M; s.Kp = (int)b.Kp; s.n_tiles = (int)b.n_tiles;
  s.amplitude = m.amplitude; s.y_std = y_std; s.lambda = m.amplitude * m.noise; s.white = m.white;
  switch (b.nsub) {
    case 1: rc = launch_ivr_score<1>(ctx, m, s); break;
    case 2: rc = launch_ivr_score<2>(ctx, m, s); break;
    default: rc = launch_ivr_score<4>(ctx, m, s); break;
  }
  if (rc) return rc;
  ivr_mark(ctx, 2);      // stage 3, the selection, is the caller's; it records event 3 behind it (ivr_mark_end)
  return GPBO_OK;
}

void ivr_mark_end(gpbo_ctx* ctx) { ivr_mark(ctx, 3); }

}  // namespace gpbo
