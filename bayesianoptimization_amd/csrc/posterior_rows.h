// The posterior at ONE point with THREAD = TRAINING POINT, one workgroup of NP threads: the pieces polish_fused.hip (value and
// gradient, one local search per workgroup) and evolve.hip (value only, one differential evolution per workgroup) share.
//   * pr_lane: a lane's double in every lane; pr_load_w: W from memory into its padded LDS square;
//   * pr_kstar: k*_i = k(|x / l - X_i / l|^2) of thread i's point (the squared distance as one fma chain over the DP padded columns);
//   * pr_row_lds: v_i = (W k*)_i over row i of W in LDS (a padded square [NP][NP + 1]), four accumulators;
//   * pr_rows_mem: the same with W in memory: threads tid < NP / 2 walk rows 2 tid, 2 tid + 1 of W through its transposed copy
//     Wt (coalesced 16-byte loads, PR_INFLIGHT in flight per lane), wave w only up to column 128 (w + 1) (the zeros of the
//     triangle are never loaded); v lands in vs[] (zero beyond N) — the caller synchronises before reading it.
// Every sum has a fixed order: both kernels give the same bits for the same point.
#pragma once

#include "gpbo_internal.h"

namespace gpbo {

#ifndef GPBO_PR_INFLIGHT
#define GPBO_PR_INFLIGHT 16
#endif
constexpr int PR_INFLIGHT = GPBO_PR_INFLIGHT;      // 16-byte loads in flight per lane in the walks over W in memory (128 is a multiple)

__device__ __forceinline__ double pr_lane(double v, int i) {      // v of lane i (i uniform), in every lane
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), i);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), i);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}

// Wl [NP][NP + 1] = W [NP][NP] (blockDim.x == NP): coalesced rows of the matrix in memory, zeros above the diagonal included
__device__ __forceinline__ void pr_load_w(double* Wl, const double* W, int NP, int tid) {
  for (int e = tid; e < NP * NP; e += NP) {
    const int i = e / NP, k = e - i * NP;
    Wl[i * (NP + 1) + k] = W[e];
  }
}

template <int KERNEL>
__device__ __forceinline__ double pr_kstar(const double* xs, const double* xr, int DP, double& d2_out) {
  double d2 = 0.0;
  for (int t = 0; t < DP; ++t) {
    const double df = xs[t] - xr[t];
    d2 = fma(df, df, d2);
  }
  d2_out = d2;
  return gpbo_kernel_value<KERNEL>(d2);
}

__device__ __forceinline__ double pr_row_lds(const double* wrow, const double* ks, int NP) {
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  for (int k = 0; k < NP; k += 4) {
    v0 = fma(wrow[k], ks[k], v0);
    v1 = fma(wrow[k + 1], ks[k + 1], v1);
    v2 = fma(wrow[k + 2], ks[k + 2], v2);
    v3 = fma(wrow[k + 3], ks[k + 3], v3);
  }
  return (v0 + v1) + (v2 + v3);
}

// (the order of every sum is the same for any even INFLIGHT dividing 128: a0 / b0 take the even k, a1 / b1 the odd k, in order)
template <int INFLIGHT = PR_INFLIGHT>
__device__ __forceinline__ void pr_rows_mem(const double* __restrict__ Wt, const double* ks, int NP, int N, int tid, int wave,
                                            double* vs) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const int ld2 = NP / 2;
  if (tid < ld2) {
    const d2* __restrict__ wt = reinterpret_cast<const d2*>(Wt) + tid;      // Wt[k][2 tid .. 2 tid + 1] = W[2 tid ..][k]
    const int kend = min(NP, 128 * (wave + 1));
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    for (int k = 0; k < kend; k += INFLIGHT) {
      d2 w[INFLIGHT];
#pragma unroll
      for (int e = 0; e < INFLIGHT; ++e) w[e] = wt[(int64_t)(k + e) * ld2];
#pragma unroll
      for (int e = 0; e < INFLIGHT; e += 2) {
        a0 = fma(w[e].x, ks[k + e], a0);
        b0 = fma(w[e].y, ks[k + e], b0);
        a1 = fma(w[e + 1].x, ks[k + e + 1], a1);
        b1 = fma(w[e + 1].y, ks[k + e + 1], b1);
      }
    }
    vs[2 * tid] = (2 * tid < N) ? a0 + a1 : 0.0;
    vs[2 * tid + 1] = (2 * tid + 1 < N) ? b0 + b1 : 0.0;
  }
}

// Wt = W^T made once per fit into the slot's K buffer (a fit assembles K straight into L; gpbo_get_K and the LML path, which write
// K, clear m.wt_valid).  Defined in polish_fused.hip with its kernel: a __global__ function needs one translation unit.
int ensure_w_transposed(gpbo_ctx* ctx, Model& m);

}  // namespace gpbo
