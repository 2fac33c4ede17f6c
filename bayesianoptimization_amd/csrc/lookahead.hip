// Two-step lookahead expected improvement (Ginsbourger & Le Riche 2010; Wu & Frazier 2019) over the resident candidates (gfx950):
// gpla_ei2_argbest's values.  include/gpla.h has the formulas, the conventions and the order of every sum; lookahead_plan.h the LDS
// layout, its budget and the workspace.  Per candidate x, reference points a_1 .. a_J, point 0 the candidate itself, Gauss-Hermite
// nodes (z_h, omega_h):
//   cov_j(x) = c (k(x, a_j) + sum_i k(x, X_i) V_j,i),      V_j = -K'^-1 k*(a_j)
//   g_j = cov_j / den,  q_j = sqrt(max(p_j - g_j^2, 0)),   b_h = max(bn, mn + den z_h)
//   t_h = max_j G(m_j + g_j z_h, q_j, b_h),                 ys[x] = -(y_std (G(mn, den, bn) + sum_h omega_h t_h))
// with G(mean, sd, a) = E[(Y - a)^+] (acq_formulas.h: ehvi_g_dev).  An (M x N) (N x J) product with H (J + 1) Phi / phi evaluations
// per candidate behind it: at J = 64, H = 16 the epilogue is 1040 of them, as much work as the product.  Neither an M x J nor an
// M x H block exists in memory.  Compiled with -ffp-contract=off, as jes.hip.
//
// Three stages:
//   points   jes.hip's (launch_jes_points): k*(a_j), the solves V_j, m_j and p_j, the fragment-packed V — the same kernels, the same
//            bits.
//   score    la_score_kernel, the hot path.  The product is jes.hip's too (jes_product.h): four waves over 64 candidates, k* generated
//            into LDS, the waves sharing a fragment by jes_split(J).  It leaves cov [64][P] in LDS, and the epilogue is where this
//            kernel is its own.  One thread per candidate, as kg.hip's envelope has it, would leave three waves in four idle through
//            a thousand transcendental chains; one thread per (candidate, point, node) would take sqrt and the division H times over.
//            So the epilogue runs in three phases, the thread's lane always the candidate:
//              A  thread = (candidate, points j = wave mod 4): g_j in place of cov_j, q_j into the twin tile; wave 0 also point 0.
//                 One division and one sqrt per (candidate, point), none per node.
//              B  thread = (candidate, nodes h = wave mod 4): b_h once, then j = 0 .. J with a running maximum over G, two LDS reads
//                 per evaluation (m_j is the same word for the whole wave), t_h into T.  All 256 threads carry evaluations whenever
//                 H >= 4; lanes DIVERGE over G's two ranges, as mes.hip's do over h's.
//              C  threads 0 .. 63: e1, the weighted sum h ascending, the NaN conventions, the store.
//            The tiles' odd pitches put a wave's 64 candidates on 64 banks.  No array lives in registers under a run-time index.
//   select   the existing arg-best / top-k over ctx->ys (acq_kernels.hip), from the entry point.
// A candidate's bits depend on J (through the split) and on H; neither on M, nor on the grid, nor on the other candidates.  Rows
// from M on repeat row M - 1 and are not written.
#include "gpbo_internal.h"
#include "acq_formulas.h"
#include "jes_product.h"
#include "lookahead_plan.h"

#include <cmath>

namespace gpbo {

static_assert(LA_POINTS == GPLA_MAX_POINTS && LA_NODES == GPLA_MAX_NODES && LA_POINTS == JES_STAR, "one limit, three names");

struct LaScoreArgs {
  const double* Xs;       // [NP][DP] scaled train points
  const double* Vp;       // fragment-packed V (jes_plan.h), Kp * 16 * nf doubles
  const double* P;        // [>= M][DP] the scaled candidates
  const double* As;       // [64][DP] the scaled points, zero rows from J on
  const double* star;     // [5][64] (jes_star_kernel): rows 0 and 1 are m_j and p_j before the clamp
  const double* nodes;    // [32] z_h | [32] omega_h
  const double* mu;
  const double* sd;
  double* ys;
  int64_t M;
  int Kp, J, H, nf;
  double amplitude, y_mean, y_std, lambda, white, bn;
};

template <int DP, int KERNEL, int SPLIT>
__global__ __launch_bounds__(256) void la_score_kernel(const LaScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) double la_lds[];
  __shared__ double pts[2][LA_POINTS];      // m_j | p_j
  __shared__ double nod[2][LA_NODES];       // z_h | omega_h
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // the same in every lane: the loops below run on scalars
  const int64_t m0 = (int64_t)blockIdx.x * JES_ROWS;
  if (tid < 2 * LA_POINTS) {                // read behind the product's barriers
    const double v = a.star[tid];
    pts[wave][lane] = (wave == 1 && v < 0.0) ? 0.0 : v;
  } else if (tid < 2 * LA_POINTS + 2 * LA_NODES) {
    const int e = tid - 2 * LA_POINTS;
    nod[e >> 5][e & 31] = (e & 31) < a.H ? a.nodes[e] : 0.0;
  }
  const int64_t mrow = jes_product<DP, KERNEL, SPLIT>(a.Xs, a.Vp, a.P, a.As, a.M, a.Kp, a.nf, la_lds);
  const int P = la_tile_pitch(a.nf), PH = la_node_pitch(a.H);
  double* G = la_lds + lane * P;
  double* Q = la_lds + la_q_offset(DP, a.nf) + lane * P;
  double* T = la_lds + la_t_offset(DP, a.nf);
  const double mean = a.mu[mrow], sd = a.sd[mrow];
  const double qv = sd / a.y_std;
  const double v = qv * qv;
  double vl = v - a.white;
  vl = vl < 0.0 ? 0.0 : vl;
  const double vo = (v + a.lambda) - a.white;
  const double den = sqrt(vo);
  const double mn = (mean - a.y_mean) / a.y_std;
  // A: thread (wave, lane) = candidate `lane`, columns wave, wave + 4, ...; column j holds point j + 1, column J point 0
  for (int j = wave; j < a.J; j += 4) {
    const double cov = a.amplitude * G[j];
    const double g = den == 0.0 ? 0.0 : cov / den;
    double qq = pts[1][j] - g * g;
    qq = qq < 0.0 ? 0.0 : qq;
    G[j] = g;
    Q[j] = sqrt(qq);
  }
  if (wave == 0) {      // point 0, the candidate itself: m_0 = mn, p_0 = cov_0 = vl
    const double g = den == 0.0 ? 0.0 : vl / den;
    double qq = vl - g * g;
    qq = qq < 0.0 ? 0.0 : qq;
    G[a.J] = g;
    Q[a.J] = sqrt(qq);
  }
  __syncthreads();
  // B: thread (wave, lane) = candidate `lane`, nodes wave, wave + 4, ...
  const double g0 = G[a.J], q0 = Q[a.J];
  for (int h = wave; h < a.H; h += 4) {
    const double z = nod[0][h];
    const double up = mn + den * z;
    const double b = up > a.bn ? up : a.bn;
    double t = ehvi_g_dev(mn + g0 * z, q0, b);
    for (int j = 0; j < a.J; ++j) {
      const double e = ehvi_g_dev(pts[0][j] + G[j] * z, Q[j], b);
      t = (e > t || e != e) ? e : t;      // a NaN term stays
    }
    T[lane * PH + h] = t;
  }
  __syncthreads();
  // C: one thread per candidate
  if (tid >= JES_ROWS || m0 + tid >= a.M) return;
  double acc = ehvi_g_dev(mn, den, a.bn);
  for (int h = 0; h < a.H; ++h) acc = acc + nod[1][h] * T[tid * PH + h];
  const int64_t i = m0 + tid;
  if (mean != mean) { a.ys[i] = mean; return; }
  if (sd != sd) { a.ys[i] = sd; return; }
  a.ys[i] = -(a.y_std * acc);
}

template <int SPLIT>
static int launch_la_score(gpbo_ctx* ctx, const Model& m, const LaScoreArgs& a) {
  const int64_t blocks = (a.M + JES_ROWS - 1) / JES_ROWS;
  if (blocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "ei2_argbest: grid too large; shard the candidates");
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    constexpr int DP = decltype(dp)::value;
    const auto kernel = la_score_kernel<DP, decltype(k)::value, SPLIT>;
    // above 64 KiB, static part included, a workgroup has to ask: a per-device setting of this one instance, made only by the calls
    // that need it (every J > 48; J > 32 only with many nodes)
    const int lds_bytes = 8 * la_lds_doubles(DP, a.nf, a.H);
    if (la_lds_bytes(DP, a.nf, a.H) > 64 * 1024)
      GPBO_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        8 * la_lds_doubles(DP, 4, LA_NODES)));
    kernel<<<dim3((unsigned)blocks), dim3(256), (size_t)lds_bytes, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

int launch_la_values(gpbo_ctx* ctx, const Model& m, int64_t M, const double* points, int J, const double* nodes, const double* weights,
                     int H, double y_best, double y_mean, double y_std, double* mu_points_out, double* var_points_out) {
  const int d = m.d, DP = m.DP;
  int rc;
  const LaBlock b = la_block(J, d, DP, m.N, m.NP);
  if ((rc = ensure(ctx, &ctx->la, &ctx->cap_la, b.doubles))) return rc;
  double* ws = ctx->la;
  GPBO_HIP(ctx, hipMemcpyAsync(ws + b.nodes, nodes, (size_t)H * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(ws + b.weights, weights, (size_t)H * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  // stage 1: the points
  if ((rc = launch_jes_points(ctx, m, ws, b.points, points, nullptr, J, y_mean, y_std, ctx->la_clock))) return rc;
  // stage 2: the scores
  jes_mark(ctx, ctx->la_clock, 1);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  const JesBlock& p = b.points;
  LaScoreArgs s{};
  s.Xs = m.Xs; s.Vp = ws + p.Vp; s.P = ctx->Xcs; s.As = ws + p.As; s.star = ws + p.star; s.nodes = ws + b.nodes;
  s.mu = m.mu; s.sd = m.sd; s.ys = ctx->ys;
  s.M = M; s.Kp = (int)p.Kp; s.J = J; s.H = H; s.nf = p.nf;
  s.amplitude = m.amplitude; s.y_mean = y_mean; s.y_std = y_std; s.lambda = m.amplitude * m.noise; s.white = m.white;
  s.bn = (y_best - y_mean) / y_std;
  switch (p.split) {
    case 4: rc = launch_la_score<4>(ctx, m, s); break;
    case 2: rc = launch_la_score<2>(ctx, m, s); break;
    default: rc = launch_la_score<1>(ctx, m, s); break;
  }
  if (rc) return rc;
  jes_mark(ctx, ctx->la_clock, 2);      // stage 3, the selection, is the caller's; it records event 3 behind it (la_mark_end)
  if (mu_points_out || var_points_out) {
    double host[2 * JES_STAR];
    GPBO_HIP(ctx, hipMemcpyAsync(host, ws + p.star, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < J; ++t) {
      const double pj = host[JES_STAR + t] < 0.0 ? 0.0 : host[JES_STAR + t];
      if (mu_points_out) mu_points_out[t] = y_std * host[t] + y_mean;
      if (var_points_out) var_points_out[t] = (y_std * y_std) * pj;
    }
  }
  return GPBO_OK;
}

void la_mark_end(gpbo_ctx* ctx) { jes_mark(ctx, ctx->la_clock, 3); }

}  // namespace gpbo
