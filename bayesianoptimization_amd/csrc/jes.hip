// Joint entropy search, lower bound (Hvarfner, Hutter & Nardi 2022; Tu et al. 2022) over the resident candidates (gfx950):
// gpje_jes_argbest's values.  include/gpje.h has the formulas, r2's ranges and the conventions; jes_plan.h the split rule, the packing
// of V and the workspace.  Per candidate x and sampled optimum (x*_s, f*_s):
//   cov_s(x) = c (k(x, x*_s) + sum_i k(x, X_i) V_s,i),      V_s = -K'^-1 k*(x*_s)
//   mu_s = mn + cov_s g_s,  vl_s = max(vl - cov_s^2 rho_s, 0),  beta = (fn_s - mu_s) / sqrt(vl_s),  term_s = 1/2 log(vl_s r2(beta) + lambda)
//   ys[x]    = -(1/2 log(vo) - (sum_s term_s) / S)
// an (M x N) (N x S) product with a transcendental chain per entry behind it.  The M x S block exists in LDS only, 64 rows at a time.
// Compiled with -ffp-contract=off, as ivr.hip.
//
// Three stages:
//   points   jes_points_kernel (k*(x*_s) over the train points), launch_path_solve (posterior_paths.hip) with zero noise draws and a
//            zero vector for alpha leaves V_s, jes_star_kernel the samples' m_s, p_s, rho_s, g_s, fn_s, jes_pack_kernel the
//            fragment-packed image of V.  2 N^2 S flops on GEMV kernels: not the hot path.
//   score    jes_score_kernel, the hot path.  A workgroup of four waves owns 64 candidates; thread (wave w, lane l) keeps candidate
//            l's scaled coordinates in registers.  Per stage of JES_KC = 32 train points the points' rows go through LDS and come back
//            as broadcasts; wave w generates k(x_l, X_i) for the 8 points 8 w .. 8 w + 7 of the stage into the k-major LDS block
//            [32][68]: the A operand, as ivr.hip.  The product is where the two differ: S <= 64 is at most four 16-column fragments,
//            so instead of a fragment per wave the SPLIT = jes_split(S) waves that share fragment u = w / SPLIT each multiply their
//            own 8 / SPLIT k-steps of the stage into it — 64 rows x 16 columns, 16 accumulator registers per wave, and at S = 16
//            all four waves feed the matrix core where a fragment per wave would leave three multiplying zeros.  The B fragments
//            come straight from the packed V (one 512-byte line per load), requested before the stage's generation and used behind
//            it.  Behind the last stage the samples' own points take the same route once, 32 at a time, and the LAST wave of each
//            split group adds k(x_l, x*_s) through a unit B fragment: one rounding, the last term of the last partial sum.
//            Then the stage buffers are dead and become sums [64][16 NF + 1]: the split's waves store / add their accumulators in
//            wave order, a barrier between them.  The epilogue leaves the MFMA register layout: thread (w, l) takes candidate l and
//            the samples w, w + 4, ... — S / 4 entries per thread, rho_s / g_s / fn_s the same LDS word for the whole wave, the
//            sums read at the odd pitch 16 NF + 1 without a bank conflict — and writes 1/2 log(vt_s + lambda) back in place.  Lanes
//            DIVERGE over r2's ranges, as mes.hip's do over h's.  Then 64 threads add their candidate's S terms, s ascending, apply
//            1/2 log(vo) and the NaN conventions, and store ys.
//   select   the existing arg-best / top-k over ctx->ys (acq_kernels.hip), from the entry point.
// A candidate's bits depend neither on M nor on the other candidates; they depend on S through the split (include/gpje.h states the
// order of every sum).  Rows from M on repeat row M - 1 and are not written.
#include "gpbo_internal.h"
#include "acq_formulas.h"
#include "jes_plan.h"
#include "jes_product.h"
#include "jes_r2.h"

#include <cmath>

namespace gpbo {

// 1/2 log(vt_s + lambda) of one (candidate, sample); a NaN anywhere comes out as NaN (the comparisons are written to keep it)
__device__ __forceinline__ double jes_term(const double cov, const double mn, const double vl, const double rho, const double g,
                                           const double fn, const double lambda) {
  const double mu_s = mn + cov * g;
  double vls = vl - (cov * cov) * rho;
  vls = vls < 0.0 ? 0.0 : vls;
  if (vls == 0.0) return 0.5 * log(lambda);
  const double beta = (fn - mu_s) / sqrt(vls);
  return 0.5 * log(vls * jes_r2_dev(beta) + lambda);
}

// KS[s][i] = k(x*_s, X_i) for i < N, 0 up to NP.  Workgroup = sample; thread t takes the train points t, t + 256, ...
template <int DP, int KERNEL>
__global__ __launch_bounds__(256) void jes_points_kernel(const double* __restrict__ Xs, const double* __restrict__ As,
                                                         double* __restrict__ KS, int N, int NP) {
  const int s = blockIdx.x;
  double xa[DP];
#pragma unroll
  for (int t = 0; t < DP; ++t) xa[t] = As[(int64_t)s * DP + t];
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
    KS[(int64_t)s * NP + i] = kv;
  }
}

// star [5][64] = m_s | p_s | rho_s | g_s | fn_s; zeros from S on.  Workgroup = sample; thread t adds the train points t, t + 256, ...
// in order, the 256 partial sums by a fixed tree.
__global__ __launch_bounds__(256) void jes_star_kernel(const double* __restrict__ KS, const double* __restrict__ V,
                                                       const double* __restrict__ alpha, const double* __restrict__ fraw, int S, int N,
                                                       int NP, double amplitude, double y_mean, double y_std, double* __restrict__ star) {
  __shared__ double red[2][256];
  const int s = blockIdx.x, tid = threadIdx.x;
  double am = 0.0, ap = 0.0;
  if (s < S) {
    for (int i = tid; i < N; i += 256) {
      const double kv = KS[(int64_t)s * NP + i];
      am = am + alpha[i] * kv;
      ap = ap + kv * V[(int64_t)s * NP + i];
    }
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
  double m = 0.0, p = 0.0, rho = 0.0, g = 0.0, fn = 0.0;
  if (s < S) {
    m = red[0][0];
    p = amplitude * (1.0 + red[1][0]);
    fn = (fraw[s] - y_mean) / y_std;
    rho = p > 0.0 ? 1.0 / p : 0.0;
    g = rho * (fn - m);
  }
  star[s] = m;
  star[JES_STAR + s] = p;
  star[2 * JES_STAR + s] = rho;
  star[3 * JES_STAR + s] = g;
  star[4 * JES_STAR + s] = fn;
}

// V [S][NP] into the packed image (jes_plan.h), every slot of it: a sample from S on and a train point from N on are 0
__global__ void jes_pack_kernel(const double* __restrict__ V, double* __restrict__ Vp, int64_t n, int S, int N, int NP, int nf) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int lane = (int)(e & 63), ks = (int)((e >> 6) & 7);
  const int64_t gu = e >> 9;
  const int u = (int)(gu % nf);
  const int64_t i = (gu / nf) * JES_KC + 4 * ks + (lane >> 4);
  const int s = 16 * u + (lane & 15);
  Vp[e] = (s < S && i < N) ? V[(int64_t)s * NP + i] : 0.0;
}

struct JesScoreArgs {
  const double* Xs;       // [NP][DP] scaled train points
  const double* Vp;       // fragment-packed V (jes_plan.h), Kp * 16 * nf doubles
  const double* P;        // [>= M][DP] the scaled candidates
  const double* As;       // [64][DP] the scaled x*_s, zero rows from S on
  const double* star;     // [5][64] (jes_star_kernel)
  const double* mu;
  const double* sd;
  double* ys;
  int64_t M;
  int Kp, S, nf;
  double amplitude, y_mean, y_std, lambda, white;
};

template <int DP, int KERNEL, int SPLIT>
__global__ __launch_bounds__(256) void jes_score_kernel(const JesScoreArgs a) {
  constexpr int NFMAX = SPLIT == 4 ? 1 : (SPLIT == 2 ? 2 : 4);
  __shared__ __attribute__((aligned(16))) double lds[jes_lds_doubles(DP, NFMAX)];
  __shared__ double star[3][JES_STAR];      // rho_s | g_s | fn_s
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t m0 = (int64_t)blockIdx.x * JES_ROWS;
  if (tid < 3 * JES_STAR) star[tid >> 6][lane] = a.star[2 * JES_STAR + tid];      // read behind the product's barriers
  const int64_t mrow = jes_product<DP, KERNEL, SPLIT>(a.Xs, a.Vp, a.P, a.As, a.M, a.Kp, a.nf, lds);
  double* sums = lds;
  const int pitch = 16 * a.nf + 1;
  // thread (wave, lane): candidate `lane`, samples wave, wave + 4, ...
  const double mean = a.mu[mrow], sd = a.sd[mrow];
  const double qv = sd / a.y_std;
  const double v = qv * qv;
  {
    double vl = v - a.white;
    vl = vl < 0.0 ? 0.0 : vl;
    const double mn = (mean - a.y_mean) / a.y_std;
    for (int s = wave; s < a.S; s += 4) {
      double* e = sums + lane * pitch + s;
      *e = jes_term(a.amplitude * *e, mn, vl, star[0][s], star[1][s], star[2][s], a.lambda);
    }
  }
  __syncthreads();
  if (tid >= JES_ROWS || m0 + tid >= a.M) return;
  double total = 0.0;
  for (int s = 0; s < a.S; ++s) total = total + sums[tid * pitch + s];
  const int64_t i = m0 + tid;
  if (mean != mean) { a.ys[i] = mean; return; }
  if (sd != sd) { a.ys[i] = sd; return; }
  const double vo = (v + a.lambda) - a.white;
  a.ys[i] = -(0.5 * log(vo) - total / (double)a.S);
}

// debug build: an event before and after each stage of the last call on its clock (gpje_debug_stage_ms, gpla_debug_stage_ms); the
// product records nothing
void jes_mark(gpbo_ctx* ctx, StageClock& c, int i) {
#ifdef GPBO_DEBUG
  if (!c.ev[i]) (void)hipEventCreate(&c.ev[i]);
  (void)hipEventRecord(c.ev[i], ctx->stream);
  c.used = (i == c.n - 1);
#else
  (void)ctx; (void)c; (void)i;
#endif
}

template <int SPLIT>
static int launch_jes_score(gpbo_ctx* ctx, const Model& m, const JesScoreArgs& a) {
  const int64_t blocks = (a.M + JES_ROWS - 1) / JES_ROWS;
  if (blocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "jes_argbest: grid too large; shard the candidates");
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    jes_score_kernel<decltype(dp)::value, decltype(k)::value, SPLIT><<<dim3((unsigned)blocks), dim3(256), 0, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

// The points stage into the workspace ws laid out by b: k*(a_s), V_s = -K'^-1 k*(a_s), the points' scalars (jes_star_kernel) and the
// packed V, event 0 of `clock` in front of its kernels.  f_star null: the values are taken as 0 (lookahead.hip reads m_s and p_s only).
int launch_jes_points(gpbo_ctx* ctx, const Model& m, double* ws, const JesBlock& b, const double* x_star, const double* f_star, int S,
                      double y_mean, double y_std, StageClock& clock) {
  const int N = (int)m.N, NP = (int)m.NP, d = m.d, DP = m.DP;
  int rc;
  GPBO_HIP(ctx, hipMemcpyAsync(ws + b.raw, x_star, (size_t)S * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (f_star) GPBO_HIP(ctx, hipMemcpyAsync(ws + b.fraw, f_star, (size_t)S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemsetAsync(ws + b.zero, 0, (size_t)b.n_zero * sizeof(double), ctx->stream));
  if ((rc = launch_prescale(ctx, ws + b.raw, S, d, DP, m.ls, ws + b.As, JES_STAR))) return rc;
  // stage 1: k*(x*_s), V_s, the samples' scalars, the packed V
  jes_mark(ctx, clock, 0);
  rc = with_dp_kernel(ctx, DP, m.kernel, [&](auto dp, auto k) {
    jes_points_kernel<decltype(dp)::value, decltype(k)::value><<<dim3((unsigned)S), dim3(256), 0, ctx->stream>>>(m.Xs, ws + b.As,
                                                                                                                ws + b.KS, N, NP);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
  if (rc) return rc;
  if ((rc = launch_path_solve(ctx, m, S, ws + b.KS, ws + b.zero, ws + b.zero, ws + b.T, ws + b.V))) return rc;
  jes_star_kernel<<<dim3(JES_STAR), dim3(256), 0, ctx->stream>>>(ws + b.KS, ws + b.V, m.alpha, f_star ? ws + b.fraw : ws + b.zero, S, N, NP,
                                                                 m.amplitude, y_mean, y_std, ws + b.star);
  GPBO_HIP(ctx, hipGetLastError());
  jes_pack_kernel<<<dim3((unsigned)((b.n_Vp + 255) / 256)), dim3(256), 0, ctx->stream>>>(ws + b.V, ws + b.Vp, b.n_Vp, S, N, NP, b.nf);
  GPBO_HIP(ctx, hipGetLastError());
  return GPBO_OK;
}

int launch_jes_values(gpbo_ctx* ctx, const Model& m, int64_t M, const double* x_star, const double* f_star, int S, double y_mean,
                      double y_std, double* mu_star_out, double* var_star_out) {
  const int d = m.d, DP = m.DP;
  int rc;
  const JesBlock b = jes_block(S, d, DP, m.N, m.NP);
  if ((rc = ensure(ctx, &ctx->je, &ctx->cap_je, b.doubles))) return rc;
  double* ws = ctx->je;
  if ((rc = launch_jes_points(ctx, m, ws, b, x_star, f_star, S, y_mean, y_std, ctx->je_clock))) return rc;
  // stage 2: the scores
  jes_mark(ctx, ctx->je_clock, 1);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  JesScoreArgs s{};
  s.Xs = m.Xs; s.Vp = ws + b.Vp; s.P = ctx->Xcs; s.As = ws + b.As; s.star = ws + b.star; s.mu = m.mu; s.sd = m.sd; s.ys = ctx->ys;
  s.M = M; s.Kp = (int)b.Kp; s.S = S; s.nf = b.nf;
  s.amplitude = m.amplitude; s.y_mean = y_mean; s.y_std = y_std; s.lambda = m.amplitude * m.noise; s.white = m.white;
  switch (b.split) {
    case 4: rc = launch_jes_score<4>(ctx, m, s); break;
    case 2: rc = launch_jes_score<2>(ctx, m, s); break;
    default: rc = launch_jes_score<1>(ctx, m, s); break;
  }
  if (rc) return rc;
  jes_mark(ctx, ctx->je_clock, 2);      // stage 3, the selection, is the caller's; it records event 3 behind it (jes_mark_end)
  if (mu_star_out || var_star_out) {
    double host[2 * JES_STAR];
    GPBO_HIP(ctx, hipMemcpyAsync(host, ws + b.star, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < S; ++t) {
      if (mu_star_out) mu_star_out[t] = y_std * host[t] + y_mean;
      if (var_star_out) var_star_out[t] = (y_std * y_std) * host[JES_STAR + t];
    }
  }
  return GPBO_OK;
}

void jes_mark_end(gpbo_ctx* ctx) { jes_mark(ctx, ctx->je_clock, 3); }

#ifdef GPBO_DEBUG
__global__ void jes_r2_kernel(const double* __restrict__ beta, int n, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = jes_r2_dev(beta[i]);
}

int debug_jes_r2(gpbo_ctx* ctx, const double* beta, int n, double* out) {
  int rc;
  if ((rc = ensure(ctx, &ctx->je, &ctx->cap_je, 2 * (int64_t)n))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(ctx->je, beta, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  jes_r2_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream>>>(ctx->je, n, ctx->je + n);
  GPBO_HIP(ctx, hipGetLastError());
  GPBO_HIP(ctx, hipMemcpyAsync(out, ctx->je + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GPBO_OK;
}
#endif

}  // namespace gpbo
