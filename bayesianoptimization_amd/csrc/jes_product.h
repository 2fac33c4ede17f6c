// The candidate x column covariance product of jes.hip's score kernel as a device function, shared with lookahead.hip: a workgroup
// of four waves over JES_ROWS = 64 candidates, k* generated k-major into LDS per stage of JES_KC = 32 train points, the columns'
// fragment-packed V (jes_plan.h) as the B operand of v_mfma_f64_16x16x4_f64, the columns' own points as one more stage with unit
// weights, the split's partial sums added in LDS.  jes.hip's header comment has the walk; include/gpje.h the order of every sum.
// Both callers compile with -ffp-contract=off.
#pragma once

#include "gpbo_internal.h"
#include "jes_plan.h"

namespace gpbo {

typedef double je_d4 __attribute__((ext_vector_type(4)));

// wave w's 8 rows of the stage in xs -> its 8 rows of the k-major block: ab[row][candidate]
template <int DP, int KERNEL>
__device__ __forceinline__ void jes_generate(const double (&xc)[DP], const double* xs, double* ab, const int wave, const int lane) {
#pragma unroll 2
  for (int q = 0; q < JES_KC / 4; q += 2) {
    const int row = wave * (JES_KC / 4) + q;
    const double* xr = xs + row * DP;          // the same address in every lane: LDS broadcast
    double d2a = 0.0, d2b = 0.0;
#pragma unroll
    for (int t = 0; t < DP; ++t) {
      const double da = xc[t] - xr[t], db = xc[t] - xr[DP + t];
      d2a = fma(da, da, d2a);
      d2b = fma(db, db, d2b);
    }
    ab[row * JES_PITCH + lane] = gpbo_kernel_value<KERNEL>(d2a);
    ab[(row + 1) * JES_PITCH + lane] = gpbo_kernel_value<KERNEL>(d2b);
  }
}

template <int DP>
__device__ __forceinline__ void jes_stage_points(const double* __restrict__ src, double* xs, const int tid) {
  const double2* s2 = reinterpret_cast<const double2*>(src);
  double2* d2 = reinterpret_cast<double2*>(xs);
  for (int e = tid; e < JES_KC * DP / 2; e += 256) d2[e] = s2[e];
}

// sums[r][s] = k(x_r, a_s) + sum_i k(x_r, X_i) V_s,i for the workgroup's 64 candidates r (rows from M on repeat row M - 1) and the
// columns s < 16 nf, left in lds as [64][16 nf + 1] behind a barrier.  lds: jes_lds_doubles(DP, nf) doubles at least.  Xs [Kp][DP] the
// scaled train points, Vp the packed V, P [>= M][DP] the scaled candidates, As [64][DP] the columns' scaled points (zero rows past the
// last).  Returns the row this lane stands for.
template <int DP, int KERNEL, int SPLIT>
__device__ __forceinline__ int64_t jes_product(const double* __restrict__ Xs, const double* __restrict__ Vp, const double* __restrict__ P,
                                               const double* __restrict__ As, const int64_t M, const int Kp, const int nf, double* lds) {
  constexpr int KSW = 8 / SPLIT;      // k-steps of a stage this wave multiplies
  double* xs = lds;                        // the stage's train points (or 32 of the columns' own points)
  double* ab = lds + JES_KC * DP;          // k* of the stage, k-major: the A operand
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lk = lane >> 4, lc = lane & 15;
  const int u = wave / SPLIT, part = wave % SPLIT;
  const bool active = u < nf;              // wave-uniform: at split 1 a wave without a fragment only generates
  const int64_t m0 = (int64_t)blockIdx.x * JES_ROWS;
  const int64_t mrow = m0 + lane < M ? m0 + lane : M - 1;
  double xc[DP];
  {
    const double* xcp = P + mrow * DP;
#pragma unroll
    for (int t = 0; t < DP; t += 2) {
      const double2 v = *reinterpret_cast<const double2*>(xcp + t);
      xc[t] = v.x;
      xc[t + 1] = v.y;
    }
  }
  je_d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = je_d4{0.0, 0.0, 0.0, 0.0};
  const double* vp = Vp + ((int64_t)(active ? u : 0) * 8 + part * KSW) * 64 + lane;
  const int64_t stage_stride = (int64_t)nf * 8 * 64;
  for (int kc = 0; kc < Kp; kc += JES_KC) {
    // this stage's B fragments: asked for now, used behind the generation
    double vb[KSW];
#pragma unroll
    for (int ks = 0; ks < KSW; ++ks) vb[ks] = active ? vp[ks * 64] : 0.0;
    vp += stage_stride;
    jes_stage_points<DP>(Xs + (int64_t)kc * DP, xs, tid);
    __syncthreads();      // xs is whole; every wave is done with the previous stage's ab
    jes_generate<DP, KERNEL>(xc, xs, ab, wave, lane);
    __syncthreads();      // ab is whole; everyone is done with xs
    if (active) {
#pragma unroll
      for (int ks = 0; ks < KSW; ++ks) {
        const double* ar = ab + ((part * KSW + ks) * 4 + lk) * JES_PITCH + lc;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[16 * t], vb[ks], acc[t], 0, 0, 0);
      }
    }
  }
  // the columns' own points, 32 at a time: row r of block q is column 32 q + r, fragment 2 q + (r >> 4)
  for (int q = 0; q < (nf + 1) / 2; ++q) {
    jes_stage_points<DP>(As + (int64_t)q * JES_KC * DP, xs, tid);
    __syncthreads();
    jes_generate<DP, KERNEL>(xc, xs, ab, wave, lane);
    __syncthreads();
    if (active && part == SPLIT - 1 && (u >> 1) == q) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double unit = (4 * j + lk == lc) ? 1.0 : 0.0;      // B[k][column] = 1 where "train point" k is the column's own point
        const double* ar = ab + (16 * (u & 1) + 4 * j + lk) * JES_PITCH + lc;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[16 * t], unit, acc[t], 0, 0, 0);
      }
    }
  }
  __syncthreads();      // xs and ab are dead: the same LDS is now sums [64][pitch]
  double* sums = lds;
  const int pitch = 16 * nf + 1;
#pragma unroll
  for (int pp = 0; pp < SPLIT; ++pp) {
    if (active && part == pp) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double* dst = sums + (16 * t + 4 * r + lk) * pitch + 16 * u + lc;
          *dst = pp == 0 ? acc[t][r] : *dst + acc[t][r];
        }
      }
    }
    __syncthreads();
  }
  return mrow;
}

}  // namespace gpbo
