// Knowledge gradient (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011) over the resident candidates (gfx950):
// gpbo_kg_argbest's values.  include/gpbo.h has the formulas and the conventions.  Per candidate x and reference point a_j:
//   cov_j(x) = c (k(x, a_j) + sum_i k(x, X_i) V_j,i),      V_j = -W^T (W k*(a_j)) = -K'^-1 k*(a_j)
//   lines (a_0, b_0) = (mu(x), y_std max(v - w, 0) / den),  (a_j, b_j) = (mu_j, y_std cov_j(x) / den),  den = sqrt(v + lambda - w)
//   ys[i] = -(E_Z[max_j (a_j + b_j Z)] - max_j a_j)
// Compiled with -ffp-contract=off, as acq_kernels.hip: acq_formulas.h's pieces give the bits they give there (the fmas below are
// written out).
//
// Three stages:
//   kg_points_kernel   a workgroup per point: k*(a_j) over the train points, mu_j.  Then launch_path_solve (posterior_paths.hip, the
//                      kernels gpbo_sample_paths solves its columns with) with zero noise draws and a zero vector for alpha leaves
//                      V_j.  2 N^2 J flops, not the hot path.
//   kg_cov_kernel      the hot path, a sibling of path_eval_kernel: thread = candidate with its coordinates in registers, the train
//                      points staged through LDS 64 at a time and read back as broadcasts, one fma per (kernel value, point
//                      column), NS columns per pass held in registers (indexed by unrolled loops only); the points of the pass are
//                      one more stage with unit weights.  blockIdx.y = the pass: J > NS repeats the k* generation per group of NS
//                      columns.  Writes cov [J][M].  A column's sum runs i = 0 .. N - 1 whatever NS, M and the grid are.
//   kg_value_kernel    thread = candidate: the J + 1 lines into LDS, kg_lines_value, ys.
//
// kg_lines_value keeps a thread's lines in LDS as [line][thread] (consecutive lanes = consecutive words: no bank conflicts, and
// every thread touches its own column only, so there is no barrier in it).  A per-thread array indexed by a run-time value would
// live in scratch, which no product kernel may use; 65 lines x 2 doubles x 64 threads are 66,560 bytes, two workgroups of one wave
// per compute unit at J = 64 and nine at J = 16.  The sort is in place and the envelope's stack is built in place over the sorted
// lines (the stack never outgrows the read position), with breakpoints recomputed from neighbours instead of stored: a third array
// would cost occupancy to save a division per pop.
//
// LOOP BOUNDS of kg_lines_value, n = n_lines <= GPBO_MAX_KG_POINTS + 1, whatever the data (a comparison with NaN is false, and a set
// with a NaN or infinite entry leaves after the first scan anyway): the scan n; the insertion sort's outer loop n - 1 and its inner
// loop at most i shifts for line i (n (n - 1) / 2 in all); the envelope's outer loop n, one push each at most, and its pop loop is a
// counted loop of at most s - 1 < n iterations per line and pops at most n - 1 lines in all, since every pop removes a pushed line;
// the final sum at most n - 1 terms.
#include "gpbo_internal.h"
#include "acq_formulas.h"

#include <cmath>

namespace gpbo {

constexpr int KG_CH = 64;          // train points per LDS stage
constexpr int KG_VT = 64;          // threads (candidates) per workgroup of kg_value_kernel
constexpr int KG_MAX_LINES = GPBO_MAX_KG_POINTS + 1;
constexpr size_t KG_VALUE_LDS_MAX = (size_t)KG_MAX_LINES * 2 * KG_VT * sizeof(double);
constexpr double KG_F_ZERO_BELOW = -40.0;      // phi(-40) and Phi(-40) are 0 in fp64 (and -inf * 0 is kept out)

// The call's workspace (ctx->kg), offsets in doubles:
//   raw (J, d) | As [64][DP] | zero [max(J N, NP)] | KS [J][NP] | T [J][NP] | V [J][NP] | mu_pts [64] | cov [J][M]
// cov is the large one: 8 J M bytes (512 MiB at J = 64, M = 2^20), kept by the context until gpbo_destroy like its other workspaces.
struct KgBlock { int64_t raw, As, zero, n_zero, KS, T, V, mu_pts, cov, doubles; };
static KgBlock kg_block(int64_t J, int64_t d, int64_t DP, int64_t N, int64_t NP, int64_t M) {
  KgBlock b{};
  b.raw = 0;
  b.As = round_up(J * d, 2);
  b.zero = b.As + GPBO_MAX_KG_POINTS * DP;
  b.n_zero = J * N > NP ? J * N : NP;
  b.KS = b.zero + round_up(b.n_zero, 2);
  b.T = b.KS + J * NP;
  b.V = b.T + J * NP;
  b.mu_pts = b.V + J * NP;
  b.cov = b.mu_pts + GPBO_MAX_KG_POINTS;
  b.doubles = b.cov + J * M;
  return b;
}

// KS[j][i] = k(a_j, X_i) for i < N, 0 up to NP; mu_pts[j] = y_std sum_i alpha_i KS[j][i] + y_mean.  Workgroup = point; thread t takes
// the train points t, t + 256, ... in order, the 256 partial sums are added by a fixed tree.
template <int DP, int KERNEL>
__global__ __launch_bounds__(256) void kg_points_kernel(const double* __restrict__ Xs, const double* __restrict__ As,
                                                        const double* __restrict__ alpha, double* __restrict__ KS,
                                                        double* __restrict__ mu_pts, int N, int NP, double y_mean, double y_std) {
  __shared__ double red[256];
  const int j = blockIdx.x;
  double xa[DP];
#pragma unroll
  for (int t = 0; t < DP; ++t) xa[t] = As[(int64_t)j * DP + t];
  double acc = 0.0;
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
      acc = fma(alpha[i], kv, acc);
    }
    KS[(int64_t)j * NP + i] = kv;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) mu_pts[j] = fma(y_std, red[0], y_mean);
}

struct KgCovArgs {
  const double* Xs;       // [NP][DP] scaled train points
  const double* V;        // [J][NP] -K'^-1 k*(a_j), zero from row N on
  const double* P;        // [>= M][DP] the scaled candidates
  const double* As;       // [64][DP] the scaled points, zero rows from J on
  double* cov;            // [J][M]
  int64_t M;
  int N, NP, J;
  double amplitude;
};

// NS = columns (accumulators) per pass; blockIdx.y = the pass, columns j0 = blockIdx.y * NS ... (those from J on are zero columns
// and are not written).
template <int DP, int KERNEL, int NS>
__global__ __launch_bounds__(256) void kg_cov_kernel(const KgCovArgs a) {
  static_assert(NS <= KG_CH, "the points of a pass are staged where a chunk of train points is");
  __shared__ __attribute__((aligned(16))) double xs[KG_CH * DP];     // train points of the stage; at the end the pass's points
  __shared__ __attribute__((aligned(16))) double wt[KG_CH * NS];     // [train point][column]
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int j0 = blockIdx.y * NS;
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
  const int k_end = (a.N + KG_CH - 1) / KG_CH * KG_CH;      // <= NP: NP is a multiple of 64
  for (int kc = 0; kc < k_end; kc += KG_CH) {
    __syncthreads();
    {
      const double2* src = reinterpret_cast<const double2*>(a.Xs + (int64_t)kc * DP);
      double2* dst = reinterpret_cast<double2*>(xs);
      for (int e = threadIdx.x; e < KG_CH * DP / 2; e += blockDim.x) dst[e] = src[e];
      for (int e = threadIdx.x; e < KG_CH * NS; e += blockDim.x) {
        const int c = e / KG_CH, kk = e - c * KG_CH;      // consecutive threads = consecutive entries of one column
        const int i = kc + kk;
        wt[kk * NS + c] = (j0 + c < a.J && i < a.N) ? a.V[(int64_t)(j0 + c) * a.NP + i] : 0.0;
      }
    }
    __syncthreads();
    if (!live) continue;
#pragma unroll 2
    for (int kk = 0; kk < KG_CH; kk += 2) {
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
  // the pass's own points: one more stage, unit weights
  __syncthreads();
  for (int e = threadIdx.x; e < NS * DP; e += blockDim.x) xs[e] = a.As[(int64_t)j0 * DP + e];     // j0 + NS <= 64 rows exist
  __syncthreads();
  if (!live) return;
  // (a counted loop over the points with the accumulator picked by an unrolled compare: NS x DP unrolled bodies are more than the
  // compiler unrolls at NS = DP = 64, and an accumulator indexed by a loop counter would leave the registers)
  const int n_cols = a.J - j0 < NS ? a.J - j0 : NS;      // the same for every thread of the grid row
#pragma unroll 1
  for (int p = 0; p < n_cols; ++p) {
    const double* xr = xs + p * DP;
    double d2 = 0.0;
#pragma unroll
    for (int t = 0; t < DP; ++t) {
      const double df = xc[t] - xr[t];
      d2 = fma(df, df, d2);
    }
    const double kv = gpbo_kernel_value<KERNEL>(d2);
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = (c == p) ? fma(kv, 1.0, acc[c]) : acc[c];
  }
#pragma unroll
  for (int c = 0; c < NS; ++c)
    if (c < n_cols) a.cov[(int64_t)(j0 + c) * a.M + m] = a.amplitude * acc[c];
}

// f(z) = phi(z) + z Phi(z) for z <= 0
__device__ __forceinline__ double kg_f_dev(double z) {
  if (z < KG_F_ZERO_BELOW) return 0.0;
  return norm_pdf_dev(z) + z * ndtr_dev(z);
}

// E_Z[max_l (A_l + B_l Z)] - max_l A_l of the n lines A[l * stride], B[l * stride] (LDS, this thread's column; overwritten).  NaN for
// a set with a NaN or infinite entry.  Loop bounds: the header.
__device__ __forceinline__ double kg_lines_value(double* A, double* B, const int n, const int stride) {
  bool finite = true;
  for (int l = 0; l < n; ++l) {
    const double av = A[l * stride], bv = B[l * stride];
    finite = finite && (fabs(av) < INFINITY) && (fabs(bv) < INFINITY);      // false for NaN
  }
  if (!finite) return NAN;
  // order by (slope, intercept): what follows sees the same sequence however the lines arrived
  for (int i = 1; i < n; ++i) {
    const double ka = A[i * stride], kb = B[i * stride];
    int j = i;
    for (; j > 0; --j) {
      const double pa = A[(j - 1) * stride], pb = B[(j - 1) * stride];
      if (!(pb > kb || (pb == kb && pa > ka))) break;
      A[j * stride] = pa;
      B[j * stride] = pb;
    }
    A[j * stride] = ka;
    B[j * stride] = kb;
  }
  // the upper envelope, its stack in place in lines 0 .. s - 1 (s <= i: line i has been read before slot s is written)
  int s = 0;
  for (int i = 0; i < n; ++i) {
    const double ai = A[i * stride], bi = B[i * stride];
    if (i + 1 < n && B[(i + 1) * stride] == bi) continue;      // a later line of the same slope has an intercept at least as large
    const int pops = s - 1;
    for (int p = 0; p < pops; ++p) {
      const double a1 = A[(s - 1) * stride], b1 = B[(s - 1) * stride];
      const double a2 = A[(s - 2) * stride], b2 = B[(s - 2) * stride];
      const double c_top = (a2 - a1) / (b1 - b2);      // where the top took over from the one below it
      const double c_new = (a1 - ai) / (bi - b1);      // where line i takes over from the top
      if (!(c_new <= c_top)) break;
      --s;      // the top is nowhere the maximum
    }
    A[s * stride] = ai;
    B[s * stride] = bi;
    ++s;
  }
  double kg = 0.0;
  for (int k = 1; k < s; ++k) {
    const double a1 = A[k * stride], b1 = B[k * stride];
    const double a0 = A[(k - 1) * stride], b0 = B[(k - 1) * stride];
    const double db = b1 - b0;
    const double c = (a0 - a1) / db;
    kg = kg + db * kg_f_dev(-fabs(c));
  }
  return kg;
}

struct KgValueArgs {
  const double* mu;
  const double* sd;
  const double* cov;      // [J][M]
  const double* mu_pts;   // [J]
  double* ys;
  int64_t M;
  int J;
  double y_std, lambda, white;
};

// -KG(x_i).  den == 0: nothing is learned, 0; a NaN mu or sd gives NaN.
__global__ __launch_bounds__(KG_VT) void kg_value_kernel(const KgValueArgs a) {
  extern __shared__ __attribute__((aligned(16))) double kg_lds[];
  const int64_t i = (int64_t)blockIdx.x * KG_VT + threadIdx.x;
  if (i >= a.M) return;      // no barrier below: a thread's lines are its own column
  const int n = a.J + 1;
  double* A = kg_lds + threadIdx.x;
  double* B = kg_lds + (size_t)n * KG_VT + threadIdx.x;
  const double mean = a.mu[i], sd = a.sd[i];
  if (mean != mean) { a.ys[i] = mean; return; }
  if (sd != sd) { a.ys[i] = sd; return; }
  const double q = sd / a.y_std;
  const double v = q * q;
  const double den = sqrt((v + a.lambda) - a.white);
  if (den == 0.0) { a.ys[i] = -0.0; return; }
  A[0] = mean;
  B[0] = (a.y_std * fmax(v - a.white, 0.0)) / den;
  for (int j = 0; j < a.J; ++j) {
    A[(j + 1) * KG_VT] = a.mu_pts[j];
    B[(j + 1) * KG_VT] = (a.y_std * a.cov[(int64_t)j * a.M + i]) / den;
  }
  a.ys[i] = -kg_lines_value(A, B, n, KG_VT);
}

static int kg_lds_attr(gpbo_ctx* ctx);

// debug build: an event before and after each stage of the last call (gpbo_debug_kg_stage_ms); the product records nothing
static inline void kg_mark(gpbo_ctx* ctx, int i) {
#ifdef GPBO_DEBUG
  if (!ctx->kg_ev[i]) (void)hipEventCreate(&ctx->kg_ev[i]);
  (void)hipEventRecord(ctx->kg_ev[i], ctx->stream);
  ctx->kg_ev_used = (i == 3);
#else
  (void)ctx; (void)i;
#endif
}

// columns per pass of kg_cov_kernel for J points (DESIGN.md has the measurement behind it); the debug build's GPBO_KG_NS forces one
static int kg_cov_ns(int J) {
  const int forced = env_override(dbg_env("GPBO_KG_NS"));
  if (forced == 16 || forced == 32 || forced == 64) return forced;
  return J <= 16 ? 16 : (J <= 32 ? 32 : 64);
}

template <int NS>
static int launch_kg_cov_ns(gpbo_ctx* ctx, const Model& m, const KgCovArgs& a) {
  const unsigned threads = path_eval_threads(a.M);
  const int64_t blocks = (a.M + threads - 1) / threads;
  if (blocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "kg_argbest: grid too large; shard the candidates");
  const unsigned passes = (unsigned)((a.J + NS - 1) / NS);
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    kg_cov_kernel<decltype(dp)::value, decltype(k)::value, NS><<<dim3((unsigned)blocks, passes), dim3(threads), 0, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

int launch_kg_values(gpbo_ctx* ctx, const Model& m, int64_t M, const double* points, int J, double y_mean, double y_std,
                     double* mu_points_out) {
  const int N = (int)m.N, NP = (int)m.NP, d = m.d, DP = m.DP;
  int rc;
  if ((rc = kg_lds_attr(ctx))) return rc;
  const KgBlock b = kg_block(J, d, DP, N, NP, M);
  if ((rc = ensure(ctx, &ctx->kg, &ctx->cap_kg, b.doubles))) return rc;
  double* ws = ctx->kg;
  GPBO_HIP(ctx, hipMemcpyAsync(ws + b.raw, points, (size_t)J * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemsetAsync(ws + b.zero, 0, (size_t)b.n_zero * sizeof(double), ctx->stream));
  if ((rc = launch_prescale(ctx, ws + b.raw, J, d, DP, m.ls, ws + b.As, GPBO_MAX_KG_POINTS))) return rc;
  // stage 1: k*(a_j), mu_j, V_j
  kg_mark(ctx, 0);
  rc = with_dp_kernel(ctx, DP, m.kernel, [&](auto dp, auto k) {
    kg_points_kernel<decltype(dp)::value, decltype(k)::value><<<dim3((unsigned)J), dim3(256), 0, ctx->stream>>>(
        m.Xs, ws + b.As, m.alpha, ws + b.KS, ws + b.mu_pts, N, NP, y_mean, y_std);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
  if (rc) return rc;
  if ((rc = launch_path_solve(ctx, m, J, ws + b.KS, ws + b.zero, ws + b.zero, ws + b.T, ws + b.V))) return rc;
  // stage 2: cov [J][M] over the candidates
  kg_mark(ctx, 1);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
  KgCovArgs c{};
  c.Xs = m.Xs; c.V = ws + b.V; c.P = ctx->Xcs; c.As = ws + b.As; c.cov = ws + b.cov;
  c.M = M; c.N = N; c.NP = NP; c.J = J; c.amplitude = m.amplitude;
  switch (kg_cov_ns(J)) {
    case 16: rc = launch_kg_cov_ns<16>(ctx, m, c); break;
    case 32: rc = launch_kg_cov_ns<32>(ctx, m, c); break;
    default: rc = launch_kg_cov_ns<64>(ctx, m, c); break;
  }
  if (rc) return rc;
  // stage 3: the envelopes
  kg_mark(ctx, 2);
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  KgValueArgs v{};
  v.mu = m.mu; v.sd = m.sd; v.cov = ws + b.cov; v.mu_pts = ws + b.mu_pts; v.ys = ctx->ys;
  v.M = M; v.J = J; v.y_std = y_std; v.lambda = m.amplitude * m.noise; v.white = m.white;
  const int64_t vblocks = (M + KG_VT - 1) / KG_VT;
  if (vblocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "kg_argbest: grid too large; shard the candidates");
  kg_value_kernel<<<dim3((unsigned)vblocks), dim3(KG_VT), (size_t)(J + 1) * 2 * KG_VT * sizeof(double), ctx->stream>>>(v);
  GPBO_HIP(ctx, hipGetLastError());
  kg_mark(ctx, 3);
  if (mu_points_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(mu_points_out, ws + b.mu_pts, (size_t)J * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GPBO_OK;
}

#ifdef GPBO_DEBUG
// gpbo_debug_kg_lines: thread = line set, kg_lines_value as kg_value_kernel calls it
__global__ __launch_bounds__(KG_VT) void kg_lines_debug_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t R,
                                                               int n, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double kg_lds[];
  const int64_t r = (int64_t)blockIdx.x * KG_VT + threadIdx.x;
  if (r >= R) return;
  double* A = kg_lds + threadIdx.x;
  double* B = kg_lds + (size_t)n * KG_VT + threadIdx.x;
  for (int l = 0; l < n; ++l) {
    A[l * KG_VT] = a[r * n + l];
    B[l * KG_VT] = b[r * n + l];
  }
  out[r] = kg_lines_value(A, B, n, KG_VT);
}

int debug_kg_lines(gpbo_ctx* ctx, const double* a, const double* b, int64_t R, int n_lines, double* out) {
  int rc;
  if ((rc = kg_lds_attr(ctx))) return rc;
  const int64_t n = R * n_lines;
  if ((rc = ensure(ctx, &ctx->kg, &ctx->cap_kg, 2 * n + R))) return rc;
  double *da = ctx->kg, *db = ctx->kg + n, *dout = ctx->kg + 2 * n;
  GPBO_HIP(ctx, hipMemcpyAsync(da, a, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(db, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const int64_t blocks = (R + KG_VT - 1) / KG_VT;
  kg_lines_debug_kernel<<<dim3((unsigned)blocks), dim3(KG_VT), (size_t)n_lines * 2 * KG_VT * sizeof(double), ctx->stream>>>(
      da, db, R, n_lines, dout);
  GPBO_HIP(ctx, hipGetLastError());
  GPBO_HIP(ctx, hipMemcpyAsync(out, dout, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GPBO_OK;
}
#endif

#ifdef GPBO_DEBUG
int debug_kg_stage_ms(gpbo_ctx* ctx, float* ms) {
  if (!ctx->kg_ev_used) GPBO_FAIL(ctx, GPBO_ERR_STATE, "debug_kg_stage_ms: no gpbo_kg_argbest call to report");
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 3; ++i) GPBO_HIP(ctx, hipEventElapsedTime(&ms[i], ctx->kg_ev[i], ctx->kg_ev[i + 1]));
  return GPBO_OK;
}
#endif

// 65 lines of 64 threads are 1 KiB more than the 64 KiB a workgroup gets without asking (a per-device setting: once per context)
static int kg_lds_attr(gpbo_ctx* ctx) {
  if (ctx->func_attrs & ATTR_KG) return GPBO_OK;
  GPBO_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kg_value_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)KG_VALUE_LDS_MAX));
#ifdef GPBO_DEBUG
  GPBO_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kg_lines_debug_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)KG_VALUE_LDS_MAX));
#endif
  ctx->func_attrs |= ATTR_KG;
  return GPBO_OK;
}

}  // namespace gpbo
