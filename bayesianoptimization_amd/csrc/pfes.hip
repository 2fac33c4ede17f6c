// Pareto-frontier entropy search over the resident candidates (gfx950): gppf_pfes_argbest's values, m = 2 (Suzuki et al. 2020;
// include/gppf.h has the formulas, the conventions and the order of every sum; pfes_plan.h the split of the work, the LDS budget and
// the workspace).  Compiled with -ffp-contract=off, as acq_kernels.hip: acq_formulas.h's pieces give the bits they give there.
//
// A sampled front is a staircase, and the region it dominates a union of strips (a_{k+1}, a_k] x (-inf, c_k].  Under independent
// normals the mass Z of that region and the second-moment term Q are sums over the strips of products of one-dimensional pieces —
// Phi and z phi at the strip's two levels of objective 0 and at its one level of objective 1 —, and the information gain is
// -log Z - Q / (2 Z).  No matrix product anywhere: M sum_s n_s strip evaluations of one erfc, one exp and one division per objective.
//
//   pfes_score_kernel     lane = candidate; the four waves of a workgroup serve the SAME 64 candidates and split a staged batch's
//                         draws, wave w taking s mod 4 == w.  The fronts come through LDS, PFES_BATCH draws at a time as (a_k, c_k)
//                         pairs, and a wave reads a point as one 16-byte broadcast.  The levels ROLL THROUGH REGISTERS: strip k
//                         needs levels k and k + 1 of objective 0 and the strips are consecutive, so a lane keeps (L, U, psi) of
//                         level k + 1 for strip k + 1 and evaluates exactly one new level per objective per strip.  No per-candidate
//                         level table in LDS or memory (ehvi.hip has one: its boxes name levels in any order; a staircase does not).
//                         Each wave leaves a_s of its draws in an LDS table [S][64]; behind the last batch wave 0 adds s = 0 .. S - 1
//                         in that order and divides once, so a candidate's bits do not depend on which wave had which draw
//   device-front mode     the joint draws at the first B candidates by gpbo_sample_paths' kernels (posterior_paths.hip), slot by slot
//                         and group by group as qnehvi.hip runs them, then qnehvi.hip's front kernel without a reference point
#include "greedy.h"
#include "acq_formulas.h"
#include "pfes_plan.h"

#include <cfloat>
#include <cmath>
#include <limits>
#include <string>

namespace gpbo {

static_assert(PFES_FRONT == GPBO_MAX_QNEHVI_FRONT, "the fronts are qnehvi_front_kernel's: rows of GPBO_MAX_QNEHVI_FRONT points");
static_assert(GPPF_MAX_FRONT_CANDIDATES <= GPBO_MAX_QNEHVI_BASE, "the front kernel has been run over this many pairs");

// One level of one objective for one candidate: L = Phi(z), U = 1 - Phi(z), each from the tail it is small in, psi = z phi(z), and
// up = (z >= 0), z = (level - mean) / sd.  sd == 0: the step.
__device__ __forceinline__ void pfes_level(double level, double mean, double sd, double& L, double& U, double& psi, bool& up) {
  const double z = (level - mean) / sd;
  up = z >= 0.0;
  if (sd == 0.0) {
    L = level >= mean ? 1.0 : 0.0; U = 1.0 - L; psi = 0.0;
    return;
  }
  const double t = 0.5 * erfc(fabs(z) * 0.70710678118654752440);
  const double pdf = norm_pdf_dev(z);
  L = up ? 1.0 - t : t;
  U = up ? t : 1.0 - t;
  psi = pdf == 0.0 ? 0.0 : z * pdf;
}

__global__ __launch_bounds__(PFES_THREADS) void pfes_score_kernel(const double* __restrict__ mu0, const double* __restrict__ sd0,
                                                                  const double* __restrict__ mu1, const double* __restrict__ sd1,
                                                                  int64_t M, int S, const double2* __restrict__ front,
                                                                  const int* __restrict__ size, double* __restrict__ ys) {
  extern __shared__ __attribute__((aligned(16))) double pfes_lds[];
  const int staged = S < PFES_BATCH ? S : PFES_BATCH;
  double2* stage = reinterpret_cast<double2*>(pfes_lds);                  // [staged][PFES_FRONT]
  double* terms = pfes_lds + (size_t)staged * PFES_FRONT * 2;             // [S][PFES_CANDS]
  const int lane = threadIdx.x & (PFES_CANDS - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / PFES_CANDS);
  const int64_t i = (int64_t)blockIdx.x * PFES_CANDS + lane;
  const bool live = i < M;      // a lane past M works on a standard normal and stores nothing
  const double m0 = live ? mu0[i] : 0.0, s0 = live ? sd0[i] : 1.0;
  const double m1 = live ? mu1[i] : 0.0, s1 = live ? sd1[i] : 1.0;
  const bool is_nan = m0 != m0 || s0 != s0 || m1 != m1 || s1 != s1;
  for (int b0 = 0; b0 < S; b0 += PFES_BATCH) {
    const int C = S - b0 < PFES_BATCH ? S - b0 : PFES_BATCH;
    __syncthreads();      // the stage before this one has been read
    for (int e = threadIdx.x; e < C * PFES_FRONT; e += PFES_THREADS) {
      const int tl = e / PFES_FRONT, k = e - tl * PFES_FRONT;
      if (k < size[b0 + tl]) stage[e] = front[(int64_t)(b0 + tl) * PFES_FRONT + k];
    }
    __syncthreads();
    for (int tl = wave; tl < C; tl += PFES_WAVES) {
      const int s = b0 + tl;
      const int n = size[s];                                   // the same word in every lane
      const double2* f = stage + tl * PFES_FRONT;
      double Z = 0.0, Q = 0.0;
      double Lk = 0.0, Uk = 1.0, pk = 0.0;                      // level k of objective 0
      bool up;
      if (n > 0) pfes_level(f[0].x, m0, s0, Lk, Uk, pk, up);
      for (int k = 0; k < n; ++k) {
        double Ln = 0.0, Un = 1.0, pn = 0.0;                    // level k + 1; behind the last point: -inf
        bool upn = false;
        if (k + 1 < n) pfes_level(f[k + 1].x, m0, s0, Ln, Un, pn, upn);
        double L1, U1, p1;
        pfes_level(f[k].y, m1, s1, L1, U1, p1, up);
        const double P0 = upn ? Un - Uk : Lk - Ln;
        const double G0 = pn - pk;
        const double G1 = -p1;
        Z = Z + P0 * L1;
        Q = Q + (G0 * L1 + P0 * G1);
        Lk = Ln; Uk = Un; pk = pn;
      }
      terms[s * PFES_CANDS + lane] = Z < DBL_MIN ? 0.0 : -log(Z) - Q / (2.0 * Z);
    }
  }
  __syncthreads();
  if (wave != 0 || !live) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc = acc + terms[s * PFES_CANDS + lane];
  ys[i] = is_nan ? std::numeric_limits<double>::quiet_NaN() : -(acc / (double)S);
}

int launch_pfes_values(gpbo_ctx* ctx, const Model* const* ms, int64_t M, const double* y_mean, const double* y_std, int G, int Sp,
                       int F, const double* omega, const double* phase, const double* weights, const double* eps, int n_samples,
                       const int* front_size_in, const double* fronts_in, int* front_size_out, double* fronts_out) {
  int rc;
  const bool on_device = omega != nullptr;
  const int S = on_device ? G * Sp : n_samples;
  const int64_t B = on_device ? (M < GPPF_MAX_FRONT_CANDIDATES ? M : (int64_t)GPPF_MAX_FRONT_CANDIDATES) : 0;
  const PfesBlock b = pfes_block(S, B);
  if ((rc = ensure(ctx, &ctx->pf, &ctx->cap_pf, b.doubles))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  double* w = ctx->pf;
  double2* front = (double2*)(w + b.front);
  int* size = (int*)(w + b.size);
  const size_t front_bytes = (size_t)S * PFES_FRONT * 2 * sizeof(double);
  greedy_mark(ctx, ctx->pf_clock, 0);
  if (on_device) {
    const int d = ms[0]->d, DP = ms[0]->DP;
    double* vals = w + b.vals;
    int* flag = (int*)(w + b.flag);
    const int64_t Bp = round_up(B, POST_CANDS);
    if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Bp * DP))) return rc;
    GPBO_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
    // the draws at the first B candidates, slot by slot (the candidates scaled by the slot's length scales) and group by group:
    // draw t = g Sp + s of objective j into row j S + t
    const GreedyDraws draws = greedy_draws(2, ms, G, Sp, F, omega, phase, weights, eps);
    for (int j = 0; j < 2; ++j) {
      const Model& m = *ms[j];
      if ((rc = launch_prescale(ctx, ctx->Xc, B, d, DP, m.ls, ctx->Xcs, Bp))) return rc;
      for (int g = 0; g < G; ++g) {
        PathWorkspace ws{};
        if ((rc = greedy_path_weights(ctx, draws, m, j, g, &ws))) return rc;
        const int64_t row = (int64_t)j * S + (int64_t)g * Sp;
        if ((rc = launch_paths_over(ctx, m, ws, y_mean[j], y_std[j], Sp, F, ctx->Xcs, B, vals + row * B, B))) return rc;
      }
    }
    const double none = -std::numeric_limits<double>::infinity();      // no reference point
    if ((rc = launch_qnehvi_fronts(ctx, vals, vals + (int64_t)S * B, B, (int)B, none, none, S, front, (double2*)(w + b.front0), size,
                                   (int*)(w + b.size0), flag)))
      return rc;
    int over = 0;
    GPBO_HIP(ctx, hipMemcpyAsync(&over, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (over)
      GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "pfes_argbest: the front of draw " + std::to_string(S - over) + " outgrew " +
                                               std::to_string(PFES_FRONT) + " points (GPPF_MAX_FRONT); a front is never thinned");
  } else {
    GPBO_HIP(ctx, hipMemcpyAsync(front, fronts_in, front_bytes, hipMemcpyHostToDevice, ctx->stream));
    GPBO_HIP(ctx, hipMemcpyAsync(size, front_size_in, (size_t)S * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the caller's arrays are pageable and theirs again on return
  }
  if (front_size_out) GPBO_HIP(ctx, hipMemcpyAsync(front_size_out, size, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (fronts_out) GPBO_HIP(ctx, hipMemcpyAsync(fronts_out, front, front_bytes, hipMemcpyDeviceToHost, ctx->stream));
  greedy_mark(ctx, ctx->pf_clock, 1);
  pfes_score_kernel<<<dim3((unsigned)pfes_blocks(M)), dim3(PFES_THREADS), (size_t)pfes_lds_bytes(S), ctx->stream>>>(
      ms[0]->mu, ms[0]->sd, ms[1]->mu, ms[1]->sd, M, S, front, size, ctx->ys);
  GPBO_HIP(ctx, hipGetLastError());
  greedy_mark(ctx, ctx->pf_clock, 2);
  return GPBO_OK;
}

void pfes_mark_end(gpbo_ctx* ctx) { greedy_mark(ctx, ctx->pf_clock, 3); }

}  // namespace gpbo
