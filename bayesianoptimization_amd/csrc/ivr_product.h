// The candidate x integration-point covariance product of ivr.hip as device functions: gpiv_ivr_argbest (ivr.hip) and gpls_sur_argbest
// (sur.hip) evaluate the same text up to the accumulators, so cov_j(x) has the same bits in both.  ivr.hip has the description of the
// stages, ivr_plan.h the packing of V.  Both callers compile with -ffp-contract=off (the fmas below are written out).
#pragma once

#include "gpbo_internal.h"
#include "ivr_plan.h"

namespace gpbo {

typedef double iv_d4 __attribute__((ext_vector_type(4)));

// candidate m0 + lane's scaled coordinates (rows from M on repeat row M - 1)
template <int DP>
__device__ __forceinline__ void ivr_load_candidate(const double* P, const int64_t m0, const int64_t M, const int lane, double (&xc)[DP]) {
  const int64_t m = m0 + lane < M ? m0 + lane : M - 1;
  const double* xcp = P + m * DP;
#pragma unroll
  for (int t = 0; t < DP; t += 2) {
    const double2 v = *reinterpret_cast<const double2*>(xcp + t);
    xc[t] = v.x;
    xc[t + 1] = v.y;
  }
}

// wave w's 8 rows of the stage in xs -> its 8 rows of the k-major block: ab[row][candidate]
template <int DP, int KERNEL>
__device__ __forceinline__ void ivr_generate(const double (&xc)[DP], const double* xs, double* ab, const int wave, const int lane) {
#pragma unroll 2
  for (int q = 0; q < IVR_KC / 4; q += 2) {
    const int row = wave * (IVR_KC / 4) + q;
    const double* xr = xs + row * DP;          // the same address in every lane: LDS broadcast
    double d2a = 0.0, d2b = 0.0;
#pragma unroll
    for (int t = 0; t < DP; ++t) {
      const double da = xc[t] - xr[t], db = xc[t] - xr[DP + t];
      d2a = fma(da, da, d2a);
      d2b = fma(db, db, d2b);
    }
    ab[row * IVR_PITCH + lane] = gpbo_kernel_value<KERNEL>(d2a);
    ab[(row + 1) * IVR_PITCH + lane] = gpbo_kernel_value<KERNEL>(d2b);
  }
}

// Column tile `tile` of the product for the workgroup's 64 candidates: acc[t][u][r] = cov_j(x) / c of candidate 16 t + (lane >> 4) + 4 r
// and column 64 NSUB tile + 16 NSUB wave + 16 u + (lane & 15), the train points by k-steps of four and k(x, a_j) last.  xs
// [IVR_KC * DP] and ab [IVR_KC * IVR_PITCH] are the workgroup's LDS; every thread of it calls this, and both are free on return
// once the workgroup has passed a barrier.
template <int DP, int KERNEL, int NSUB>
__device__ __forceinline__ void ivr_tile_product(const double* __restrict__ Xs, const double* __restrict__ Vp,
                                                 const double* __restrict__ As, const int Kp, const int tile, const double (&xc)[DP],
                                                 double* xs, double* ab, iv_d4 (&acc)[4][NSUB]) {
  constexpr int KSTEPS = IVR_KC / 4;      // k-steps per stage
  constexpr int NWC = 16 * NSUB;          // columns per wave
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lk = lane >> 4, lc = lane & 15;
  const int64_t tile_stride = (int64_t)(Kp / 4) * 4 * NSUB * 64;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int u = 0; u < NSUB; ++u) acc[t][u] = iv_d4{0.0, 0.0, 0.0, 0.0};
  const double* vp = Vp + tile * tile_stride + (int64_t)wave * NSUB * 64 + lane;
  for (int kc = 0; kc < Kp; kc += IVR_KC) {
    // this stage's B fragments: asked for now, used behind the generation
    double vb[KSTEPS][NSUB];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
      for (int u = 0; u < NSUB; ++u) vb[ks][u] = vp[(ks * 4 * NSUB + u) * 64];
    vp += KSTEPS * 4 * NSUB * 64;
    {
      const double2* src = reinterpret_cast<const double2*>(Xs + (int64_t)kc * DP);
      double2* dst = reinterpret_cast<double2*>(xs);
      for (int e = tid; e < IVR_KC * DP / 2; e += 256) dst[e] = src[e];
    }
    __syncthreads();      // xs is whole; every wave is done with the previous stage's ab
    ivr_generate<DP, KERNEL>(xc, xs, ab, wave, lane);
    __syncthreads();      // ab is whole; everyone is done with xs
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const double* ar = ab + (ks * 4 + lk) * IVR_PITCH + lc;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double av = ar[16 * t];
#pragma unroll
        for (int u = 0; u < NSUB; ++u) acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, vb[ks][u], acc[t][u], 0, 0, 0);
      }
    }
  }
  // the tile's own points, 8 of the wave's columns at a time: row 8 w + q of the stage = column 16 NSUB w + 16 u + 8 h + q of the tile
  const int64_t j0 = (int64_t)tile * (4 * NWC);
#pragma unroll
  for (int u = 0; u < NSUB; ++u) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      for (int e = tid; e < IVR_KC * DP / 2; e += 256) {
        const int row = e / (DP / 2), t2 = e - row * (DP / 2);
        const int64_t j = j0 + (row >> 3) * NWC + 16 * u + 8 * h + (row & 7);
        reinterpret_cast<double2*>(xs)[e] = reinterpret_cast<const double2*>(As + j * DP)[t2];
      }
      __syncthreads();
      ivr_generate<DP, KERNEL>(xc, xs, ab, wave, lane);
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const double unit = (8 * h + 4 * s + lk == lc) ? 1.0 : 0.0;      // B[k][column] = 1 where train "point" k is the column
        const double* ar = ab + (wave * 8 + 4 * s + lk) * IVR_PITCH + lc;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[16 * t], unit, acc[t][u], 0, 0, 0);
      }
    }
  }
}

}  // namespace gpbo
