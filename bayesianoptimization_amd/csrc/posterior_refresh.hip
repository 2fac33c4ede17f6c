// gpbo_posterior_refresh's incremental route (gfx950): the resident posterior of a slot brought up to date after gpbo_fit_append
// added rows r = N_post ... N - 1 at unchanged kernel, length scale and noise, without a pass over W.
//
// The rows of W = L^-1 above an appended row do not change, so for every candidate x
//   |W k*|^2  grows by exactly  sum_r v_r(x)^2,   v_r(x) = sum_{i <= r} W[r, i] k(x, X_i),
// and the mean is k* . alpha with the new alpha.  Per candidate that is ONE k* generation — O(N d) — contracted with 1 + n_rows
// weight vectors, against the O(N^2) of the full pass:
//   mu = y_std (sum_i alpha_i k_i) + y_mean                                   (recomputed: every target's normalisation may have changed)
//   sd = y_std sqrt(max((sd_old / y_std_old)^2 - amplitude sum_r v_r^2, 0))   (`white` is already inside sd_old)
// The variance is recovered from the resident sd, so no posterior kernel has to keep anything else: one ulp of the variance.
//
// The kernel is a sibling of kstar_gen_kernel (posterior_kernel_v2.hip): thread = candidate with its coordinates in registers, the
// train points staged through LDS 64 at a time and read back as broadcasts, the kind-generic value functions of gpbo_internal.h —
// bound by the fp64 VALU work of the generation (the distance, the root, the exponential), to which each weight column adds one
// fma per element.  A workgroup holds all rows of its candidates and writes mu and sd itself: no partial sums, no second launch,
// one fixed summation order.  fp64 whatever the slot's precision.
#include "gpbo_internal.h"

namespace gpbo {

constexpr int RF_CH = 64;           // train points per LDS stage
constexpr int RF_MAX_ROWS = 16;     // appended rows one refresh takes (gpbo_fit_append's own row-path limit)

struct RefreshArgs {
  const double* Xs;      // [NP][DP] scaled train points
  const double* alpha;   // [NP]
  const double* W;       // [NP][NP]
  const double* Xcs;     // [Mp][DP] scaled candidates
  double* mu;            // [M] resident posterior: mu is overwritten, sd is read and overwritten
  double* sd;
  int* negvar;
  int64_t M;
  int N, NP, N_post;     // rows now, padded, rows the resident sd reflects
  double y_mean, y_std, y_std_old, amplitude;
};

// NC = weight columns held per train point: column 0 = alpha, column c >= 1 = row N_post + c - 1 of W (zero beyond the rows that
// were appended: a zero column adds nothing).  The accumulators are indexed by unrolled loops over NC only, so they stay registers.
template <int DP, int KERNEL, int NC>
__global__ __launch_bounds__(256) void posterior_refresh_kernel(const RefreshArgs a) {
  __shared__ __attribute__((aligned(16))) double xs[RF_CH * DP];
  __shared__ __attribute__((aligned(16))) double wt[RF_CH * NC];     // [train point][column]
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = m < a.M;
  double xc[DP];
  {
    const double* xcp = a.Xcs + (live ? m : 0) * DP;
#pragma unroll
    for (int t = 0; t < DP; t += 2) {
      const double2 v = *reinterpret_cast<const double2*>(xcp + t);
      xc[t] = v.x;
      xc[t + 1] = v.y;
    }
  }
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  const int k_end = (a.N + RF_CH - 1) / RF_CH * RF_CH;      // <= NP: NP is a multiple of 64
  for (int kc = 0; kc < k_end; kc += RF_CH) {
    __syncthreads();
    {
      const double2* src = reinterpret_cast<const double2*>(a.Xs + (int64_t)kc * DP);
      double2* dst = reinterpret_cast<double2*>(xs);
      for (int e = threadIdx.x; e < RF_CH * DP / 2; e += blockDim.x) dst[e] = src[e];
      for (int e = threadIdx.x; e < RF_CH * NC; e += blockDim.x) {
        const int c = e / RF_CH, kk = e - c * RF_CH;      // consecutive threads = consecutive entries of one row of W
        const int i = kc + kk;
        const int r = a.N_post + c - 1;
        double w = 0.0;
        if (c == 0) { if (i < a.N) w = a.alpha[i]; }
        else if (r < a.N && i <= r) w = a.W[(int64_t)r * a.NP + i];
        wt[kk * NC + c] = w;
      }
    }
    __syncthreads();
    if (!live) continue;
#pragma unroll 2
    for (int kk = 0; kk < RF_CH; kk += 2) {
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
      const double* wa = wt + kk * NC;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        acc[c] = fma(ka, wa[c], acc[c]);
        acc[c] = fma(kb, wa[NC + c], acc[c]);
      }
    }
  }
  if (!live) return;
  double ss = 0.0;
#pragma unroll
  for (int c = 1; c < NC; ++c) ss = fma(acc[c], acc[c], ss);
  const double s_old = a.sd[m] / a.y_std_old;
  double var = fma(-a.amplitude, ss, s_old * s_old);
  if (var < 0.0) {                   // as posterior_finalize_elem: NaN stays NaN, the host warns as sklearn does
    *a.negvar = 1;
    var = 0.0;
  }
  a.sd[m] = sqrt(var * (a.y_std * a.y_std));
  a.mu[m] = a.y_std * acc[0] + a.y_mean;
}

template <int NC>
static int launch_refresh_nc(gpbo_ctx* ctx, const Model& m, const RefreshArgs& a) {
  // one workgroup per 256 candidates fills the device from ~2^17 candidates on; below, single-wave workgroups spread them wider
  const unsigned threads = a.M >= (1 << 17) ? 256u : 64u;
  const int64_t blocks = (a.M + threads - 1) / threads;
  if (blocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "posterior_refresh: grid too large; shard the candidates");
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    posterior_refresh_kernel<decltype(dp)::value, decltype(k)::value, NC><<<dim3((unsigned)blocks), dim3(threads), 0, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

// The incremental route for the M resident candidates; the caller (gpbo_posterior_refresh) has checked that the slot's resident
// mu / sd are valid for them and reflect m.N_post <= m.N <= m.N_post + RF_MAX_ROWS rows at y_std m.ystd_post.
int launch_posterior_refresh(gpbo_ctx* ctx, Model& m, int64_t M, double y_mean, double y_std) {
  const int n_rows = (int)(m.N - m.N_post);
  if (n_rows < 0 || n_rows > RF_MAX_ROWS || M < 1 || M > m.cap_M)
    GPBO_FAIL(ctx, GPBO_ERR_STATE, "posterior_refresh: the slot is not refreshable");
  const int64_t Mp = round_up(M, POST_CANDS);
  int rc;
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * m.DP))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, m.d, m.DP, m.ls, ctx->Xcs, Mp))) return rc;
  RefreshArgs a{};
  a.Xs = m.Xs; a.alpha = m.alpha; a.W = m.W; a.Xcs = ctx->Xcs; a.mu = m.mu; a.sd = m.sd; a.negvar = ctx->negvar;
  a.M = M; a.N = (int)m.N; a.NP = (int)m.NP; a.N_post = (int)m.N_post;
  a.y_mean = y_mean; a.y_std = y_std; a.y_std_old = m.ystd_post; a.amplitude = m.amplitude;
  ev_begin(ctx, T_POST_MAIN);
  // column groups: alpha + 1 row (a constant-liar step), + up to 4, + up to 16
  if (n_rows <= 1) rc = launch_refresh_nc<2>(ctx, m, a);
  else if (n_rows <= 4) rc = launch_refresh_nc<5>(ctx, m, a);
  else rc = launch_refresh_nc<1 + RF_MAX_ROWS>(ctx, m, a);
  ev_end(ctx, T_POST_MAIN);
  return rc;
}

}  // namespace gpbo
