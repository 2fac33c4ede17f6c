// Stepwise uncertainty reduction for an excursion set (Bect et al. 2012; Chevalier et al. 2014) over the resident candidates (gfx950):
// gpls_sur_argbest's values.  include/gpls.h has the formulas and the conventions; sur_plan.h the workspace and the quadrature rule;
// ivr_plan.h the tiles and the packing of V.  Per candidate x and integration point a_j:
//   cov_j(x) = c (k(x, a_j) + sum_i k(x, X_i) V_j,i)                         ivr.hip's, the same text (ivr_product.h), the same bits
//   r2       = min(cov_j(x)^2 (1 / den2(x)) (1 / s_j^2), 1),   U = r2 / (1 + sqrt((1 - r2) (1 + r2)))
//   G        = (1 / pi) int_0^U exp(-h_j^2 (1 + u^2) / (1 + u)^2) / (1 + u^2) du
//   ys[x]    = -(sum_j omega_j G)
// an (M x N) (N x J) product with a bivariate normal probability per entry behind it.  The M x J block never exists: not in memory,
// not in LDS.  Compiled with -ffp-contract=off, as ivr.hip (the fmas below are written out).
//
// Three stages:
//   points   ivr.hip's (launch_ivr_points): k*(a_j), V_j, the packed V, a group of columns at a time; behind each group's solve
//            sur_stats_kernel takes m_j and s_j^2 from the group's k* and V and leaves h_j^2, 1 / s_j^2 and p_j per column.
//   score    sur_score_kernel, the hot path.  The product is ivr.hip's, tile by tile: four waves over 64 candidates, k* generated into
//            LDS, the W-free V fragments streamed, the accumulators 64 x 16 NSUB fp64 per wave.  Behind a tile's product lane
//            (lk, lc) = (lane >> 4, lane & 15) of wave w holds, per row fragment t and column fragment u, the four candidates 16 t +
//            lk + 4 r of ONE column: the column's h2, 1 / s2 and omega are three registers per u, the rows' 1 / den2 come from 64
//            words of LDS.  Per (t, u) the four entries run the quadrature side by side — four independent chains of the same
//            instructions, which is what keeps the fp64 pipe full without a second wave: U by one root and one reciprocal; per node
//            u_i = U x_i, a = 1 + u_i, b = 1 + u_i^2, ONE reciprocal 1 / (a^2 b) that gives both b / a^2 and 1 / b, the project's
//            x <= 0 exp, w_i in a running sum, the 12 nodes ascending in a rolled loop (node and weight are wave-uniform constant
//            loads).  No sin, no asin, no branch: r2 = 0 gives U = 0 and the term is an exact +0.  Then omega_j, the wave's column
//            fragments in order, the 16 columns of a fragment by a butterfly (xor 1, 2, 4, 8), the four waves in wave order through
//            LDS, the tiles in tile order: ivr.hip's reduction.  After the last tile 1 / pi, the NaN conventions, and ctx->ys.
//   select   the existing arg-best / top-k over ctx->ys (acq_kernels.hip), from the entry point.
// A candidate's bits depend neither on M nor on the other candidates: a row of the product reads its own row of A only, its
// epilogue reads its own 1 / den2 only, and every sum above has a fixed order.  Rows from M on repeat row M - 1 and are not written.
#include "gpbo_internal.h"
#include "acq_formulas.h"
#include "ivr_product.h"
#include "sur_plan.h"

#include <cmath>

namespace gpbo {

static __constant__ double sur_rule[2][SUR_NODES] = {
    {SUR_NODE_X[0], SUR_NODE_X[1], SUR_NODE_X[2], SUR_NODE_X[3], SUR_NODE_X[4], SUR_NODE_X[5], SUR_NODE_X[6], SUR_NODE_X[7], SUR_NODE_X[8],
     SUR_NODE_X[9], SUR_NODE_X[10], SUR_NODE_X[11]},
    {SUR_NODE_W[0], SUR_NODE_W[1], SUR_NODE_W[2], SUR_NODE_W[3], SUR_NODE_W[4], SUR_NODE_W[5], SUR_NODE_W[6], SUR_NODE_W[7], SUR_NODE_W[8],
     SUR_NODE_W[9], SUR_NODE_W[10], SUR_NODE_W[11]}};
static_assert(SUR_NODES == 12, "sur_rule lists the nodes one by one");

// The group's columns [g0, g0 + cols): h2 | is2 | p of column g0 + blockIdx.x from KS / V [cols][NP].  Workgroup = column; thread t
// adds the train points t, t + 256, ... in order, the 256 partial sums by a fixed tree (jes.hip's jes_star_kernel has the same sums).
__global__ __launch_bounds__(256) void sur_stats_kernel(const double* __restrict__ KS, const double* __restrict__ V,
                                                        const double* __restrict__ alpha, int N, int NP, double amplitude, double t,
                                                        double* __restrict__ h2, double* __restrict__ is2, double* __restrict__ p) {
  __shared__ double red[2][256];
  const int jl = blockIdx.x, tid = threadIdx.x;
  double am = 0.0, ap = 0.0;
  for (int i = tid; i < N; i += 256) {
    const double kv = KS[(int64_t)jl * NP + i];
    am = am + alpha[i] * kv;
    ap = ap + kv * V[(int64_t)jl * NP + i];
  }
  red[0][tid] = am;
  red[1][tid] = ap;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) {
      red[0][tid] = red[0][tid] + red[0][tid + off];
      red[1][tid] = red[1][tid] + red[1][tid + off];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double m = red[0][0];
  double s2 = amplitude * (1.0 + red[1][0]);
  s2 = s2 < 0.0 ? 0.0 : s2;
  if (s2 == 0.0) {      // the point is decided: no term, p_j 0 or 1
    h2[jl] = 0.0;
    is2[jl] = 0.0;
    p[jl] = m > t ? 1.0 : 0.0;
    return;
  }
  const double h = (m - t) / sqrt(s2);
  h2[jl] = h * h;
  is2[jl] = 1.0 / s2;
  p[jl] = ndtr_dev(h);
}

// zeros behind the J columns, up to Jp
__global__ void sur_pad_kernel(double* __restrict__ h2, double* __restrict__ is2, double* __restrict__ p, int J, int Jp) {
  const int j = J + blockIdx.x * 256 + threadIdx.x;
  if (j >= Jp) return;
  h2[j] = 0.0;
  is2[j] = 0.0;
  p[j] = 0.0;
}

// 1 / d for d in [1, 8]: v_rcp_f64 and two Newton steps (no scaling, no special cases: the argument is a^2 b of the rule)
__device__ __forceinline__ double sur_rcp(const double d) {
  double x = __builtin_amdgcn_rcp(d);
  x = fma(fma(-d, x, 1.0), x, x);
  return fma(fma(-d, x, 1.0), x, x);
}

struct SurScoreArgs {
  const double* Xs;       // [NP][DP] scaled train points
  const double* Vp;       // fragment-packed V (ivr_plan.h), Jp x Kp doubles
  const double* P;        // [>= M][DP] the scaled candidates
  const double* As;       // [Jp][DP] the scaled points, zero rows from J on
  const double* omega;    // [Jp], zero from J on
  const double* h2;       // [Jp] h_j^2, zero from J on
  const double* is2;      // [Jp] 1 / s_j^2, zero where s_j = 0 and from J on
  const double* mu;
  const double* sd;
  double* ys;
  int64_t M;
  int Kp, n_tiles;
  double amplitude, y_std, lambda, white;
};

template <int DP, int KERNEL, int NSUB>
__global__ __launch_bounds__(256) void sur_score_kernel(const SurScoreArgs a) {
  __shared__ __attribute__((aligned(16))) double xs[IVR_KC * DP];           // the stage's train points (or the tile's own points)
  __shared__ __attribute__((aligned(16))) double ab[IVR_KC * IVR_PITCH];    // k* of the stage, k-major: the A operand
  __shared__ double red[4][IVR_ROWS];
  __shared__ double idn[IVR_ROWS];        // 1 / den2 of the workgroup's candidates (0 where den2 is 0)
  constexpr int NWC = 16 * NSUB;          // columns per wave
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lk = lane >> 4, lc = lane & 15;
  const int64_t m0 = (int64_t)blockIdx.x * IVR_ROWS;
  double xc[DP];
  ivr_load_candidate<DP>(a.P, m0, a.M, lane, xc);
  if (tid < IVR_ROWS) {      // read behind the first tile's barriers
    const int64_t m = m0 + tid < a.M ? m0 + tid : a.M - 1;
    const double q = a.sd[m] / a.y_std;
    const double den2 = (q * q + a.lambda) - a.white;
    idn[tid] = den2 == 0.0 ? 0.0 : 1.0 / den2;
  }
  double total = 0.0;      // threads 0 .. 63: candidate tid's sum over the tiles so far
  for (int tile = 0; tile < a.n_tiles; ++tile) {
    iv_d4 acc[4][NSUB];
    ivr_tile_product<DP, KERNEL, NSUB>(a.Xs, a.Vp, a.As, a.Kp, tile, xc, xs, ab, acc);      // ivr_product.h
    const int64_t j0 = (int64_t)tile * (4 * NWC);
    double om[NSUB], h2[NSUB], is2[NSUB];
#pragma unroll
    for (int u = 0; u < NSUB; ++u) {
      const int64_t j = j0 + wave * NWC + 16 * u + lc;
      om[u] = a.omega[j];
      h2[u] = a.h2[j];
      is2[u] = a.is2[j];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double g[4] = {0.0, 0.0, 0.0, 0.0};      // candidates 16 t + lk + 4 r: their sums over the wave's column fragments so far
      double rd[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) rd[r] = idn[16 * t + lk + 4 * r];
#pragma unroll
      for (int u = 0; u < NSUB; ++u) {
        double U[4], s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double cov = a.amplitude * acc[t][u][r];
          double r2 = ((cov * cov) * rd[r]) * is2[u];
          r2 = r2 > 1.0 ? 1.0 : r2;      // a NaN stays
          U[r] = r2 * sur_rcp(1.0 + gpbo_sqrt_pos((1.0 - r2) * (1.0 + r2)));
          s[r] = 0.0;
        }
#pragma unroll 1
        for (int i = 0; i < SUR_NODES; ++i) {
          const double x = sur_rule[0][i], w = sur_rule[1][i];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double ui = U[r] * x;
            const double aa = (1.0 + ui) * (1.0 + ui), b = fma(ui, ui, 1.0);
            const double inv = sur_rcp(aa * b);
            s[r] = s[r] + w * (gpbo_exp_nonpos(-(h2[u] * ((b * b) * inv))) * (aa * inv));
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) g[r] = g[r] + om[u] * (s[r] * U[r]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double v = g[r];
#pragma unroll
        for (int off = 1; off <= 8; off <<= 1) v = v + __shfl_xor(v, off);
        if (lc == 0) red[wave][16 * t + lk + 4 * r] = v;
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
  a.ys[i] = -(total * 0.31830988618379067154);      // 1 / pi
}

template <int NSUB>
static int launch_sur_score(gpbo_ctx* ctx, const Model& m, const SurScoreArgs& a) {
  const int64_t blocks = (a.M + IVR_ROWS - 1) / IVR_ROWS;
  if (blocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "sur_argbest: grid too large; shard the candidates");
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    sur_score_kernel<decltype(dp)::value, decltype(k)::value, NSUB><<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

namespace {
struct SurStats {
  double t;
  double *h2, *is2, *p;
};
// launch_ivr_points' hook: the scalars of the group's columns, while KS and V hold them
int sur_after_group(gpbo_ctx* ctx, const Model& m, const double* KS, const double* V, int g0, int cols, void* user) {
  const SurStats& s = *static_cast<const SurStats*>(user);
  sur_stats_kernel<<<dim3((unsigned)cols), dim3(256), 0, ctx->stream>>>(KS, V, m.alpha, (int)m.N, (int)m.NP, m.amplitude, s.t, s.h2 + g0,
                                                                       s.is2 + g0, s.p + g0);
  GPBO_HIP(ctx, hipGetLastError());
  return GPBO_OK;
}
}  // namespace

int launch_sur_values(gpbo_ctx* ctx, const Model& m, int64_t M, const double* points, const double* weights, int J, double level,
                      double y_mean, double y_std, double* p_out, double* unc_out) {
  const int d = m.d, DP = m.DP;
  int rc;
  const SurBlock b = sur_block(J, d, DP, m.N, m.NP);
  if ((rc = ensure(ctx, &ctx->ls, &ctx->cap_ls, b.doubles))) return rc;
  double* ws = ctx->ls;
  const int Jp = (int)b.iv.Jp;
  // stage 1: ivr.hip's points stage, the columns' scalars behind each group's solve
  SurStats st{(level - y_mean) / y_std, ws + b.h2, ws + b.is2, ws + b.p};
  if ((rc = launch_ivr_points(ctx, m, ws, b.iv, points, weights, J, ctx->ls_clock, sur_after_group, &st))) return rc;
  if (Jp > J) {
    sur_pad_kernel<<<dim3((unsigned)((Jp - J + 255) / 256)), dim3(256), 0, ctx->stream>>>(st.h2, st.is2, st.p, J, Jp);
    GPBO_HIP(ctx, hipGetLastError());
  }
  // stage 2: the scores
  jes_mark(ctx, ctx->ls_clock, 1);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  SurScoreArgs s{};
  s.Xs = m.Xs; s.Vp = ws + b.iv.Vp; s.P = ctx->Xcs; s.As = ws + b.iv.As; s.omega = ws + b.iv.omega; s.h2 = st.h2; s.is2 = st.is2;
  s.mu = m.mu; s.sd = m.sd; s.ys = ctx->ys;
  s.M = M; s.Kp = (int)b.iv.Kp; s.n_tiles = (int)b.iv.n_tiles;
  s.amplitude = m.amplitude; s.y_std = y_std; s.lambda = m.amplitude * m.noise; s.white = m.white;
  switch (b.iv.nsub) {
    case 1: rc = launch_sur_score<1>(ctx, m, s); break;
    case 2: rc = launch_sur_score<2>(ctx, m, s); break;
    default: rc = launch_sur_score<4>(ctx, m, s); break;
  }
  if (rc) return rc;
  jes_mark(ctx, ctx->ls_clock, 2);      // stage 3, the selection, is the caller's; it records event 3 behind it (sur_mark_end)
  if (p_out || unc_out) {
    // p_j and omega_j of the J points; the uncertainty is their sum on the host, j ascending
    std::vector<double> host(2 * (size_t)J);
    GPBO_HIP(ctx, hipMemcpyAsync(host.data(), st.p, (size_t)J * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipMemcpyAsync(host.data() + J, ws + b.iv.omega, (size_t)J * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double unc = 0.0;
    for (int j = 0; j < J; ++j) {
      const double p = host[j];
      if (p_out) p_out[j] = p;
      unc += host[J + j] * (p * (1.0 - p));
    }
    if (unc_out) *unc_out = unc;
  }
  return GPBO_OK;
}

void sur_mark_end(gpbo_ctx* ctx) { jes_mark(ctx, ctx->ls_clock, 3); }

}  // namespace gpbo
