// gpbo_polish_seeds as ONE launch: one workgroup per local search, the evaluations AND the optimiser inside it.
//
// What it replaces: the local-search stage of AcquisitionFunction._smart_minimize (bayes_opt/acquisition.py:322-420) for the
// sizes where it is launch latency and nothing else.  polish.hip advances all runs in lockstep, one batched evaluation per round:
// six dependent launches and a stream synchronisation (41-75 us) for ~2 N^2 flops per run.  Here a run is a workgroup that owns
// its search from the seed to the stopping rule, THREAD = TRAINING POINT (polish_rows_kernel, round 6):
//   * thread i keeps k*_i, v_i = (W k*)_i and u_i = (W^T v)_i of its own point: it walks row i of W = L^-1 for v and column i for u;
//   * NP <= 128: W sits in LDS as a padded square ([NP][NP + 1]: both walks conflict-free).  128 < NP <= 512: W stays in memory and
//     both walks are coalesced — the row walk over a transposed copy made once per fit, the column walk over W itself;
//   * the sums over the points (mu, |v|^2, the 2 d gradient sums) are taken by lane groups of one dimension each and combined in a
//     fixed order; the optimiser (polish_opt.h's steps) runs on wave 0 with a lane per variable, its sums over the variables as
//     DPP row reductions, its two-loop recursion as ONE rolled loop;
//   * four barriers per evaluation.  3.4-3.9 us per evaluation at N <= 64, 5.3-5.7 at 128, 16 / 21 / 31 / 41 at N = 143 / 256 / 384 / 512
//     (one CU streams W at ~30 B per clock), against 14 / 19 / 24-46 for round 5's eight-wave kernel and 41-57 us per lockstep
//     round (profiles/r06_polish_fused_ab.json).
// Deterministic, and NOT the bits of the lockstep path (other summation orders): the evaluation agrees with gpbo_predict_grad to
// ~3e-12 of the values' scale, a whole search ends at the same or a better value ("parity is statistical
// (same or better acquisition value), not bit-wise"); the lockstep path is the checker (tests/test_gpu_polish_fused.py).  Round 5's
// eight-wave kernel — the six kernels' arithmetic phase by phase, bitwise the lockstep path, nine barriers and two passes over W
// at 25 GB/s per evaluation — is in the git history; every size it served is served faster here.
// One model (no constraint slots).  Which models are served, the kernel's LDS layout and the pinned block's: search_plan.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "gpbo_internal.h"
#include "polish_lane_opt.h"      // the optimiser on wave 0, lane = variable (pr_advance), shared with path_ascent.hip
#include "polish_opt.h"
#include "posterior_rows.h"

namespace gpbo {

namespace {

struct PolishFusedArgs {
  const double *W, *Wt, *Xs, *alpha, *ls;      // Wt: W transposed, row-major (polish_rows_kernel with W in memory), else null
  int NP, N, d, DP;
  double y_mean, y_std;
  double amplitude, white;             // of the model: normalised variance = amplitude * (1 - |W k*|^2) + white
  int acq;
  double acq_param, y_max;
  int max_iter, eval_only;             // eval_only = R > 0: R evaluations at the seed, no search (debug entry)
  const double *seeds, *lo, *hi;      // (n_seeds, d), (d,), (d,): device-visible pinned host memory
  double *x_out, *f_out;              // (n_seeds, d), (n_seeds,): pinned
  int *status_out, *iter_out, *eval_out;
  double* dbg;                        // eval_only: per seed [f, mu, sd, 0 | g (d) | dmu (d) | dsd (d)]
  int* negvar;
};

struct DevCdf {
  __device__ __forceinline__ double operator()(double z) const { return 0.5 * erfc(-z * 0.70710678118654752440); }
};
struct DevPdf {
  __device__ __forceinline__ double operator()(double z) const { return exp(-0.5 * z * z) * 0.39894228040143267794; }
};

// Wt = W^T (both row-major NP x NP, NP a multiple of 64): one 64x64 tile per 256-thread workgroup through a padded LDS image
__global__ __launch_bounds__(256) void transpose_w_kernel(const double* __restrict__ W, double* __restrict__ Wt, int NP) {
  __shared__ double tile[64][65];
  const int bi = (int)blockIdx.y, bj = (int)blockIdx.x, c = (int)threadIdx.x & 63, r0 = (int)threadIdx.x >> 6;
  for (int r = r0; r < 64; r += 4) tile[r][c] = W[(int64_t)(64 * bi + r) * NP + 64 * bj + c];
  __syncthreads();
  for (int r = r0; r < 64; r += 4) Wt[(int64_t)(64 * bj + r) * NP + 64 * bi + c] = tile[c][r];
}

// ---- thread = training point (NP <= 512) ---------------------------------------------------------------------------------
// (the LDS layout: search_plan.h's PolishLds)
// WLDS = false (round 6, 128 < NP <= 512): W stays in memory and both walks are COALESCED: the row walk reads the transposed copy
// (Wt[k][i], lanes = consecutive i), the column walk reads W itself (W[i'][k], lanes = consecutive k), two rows (columns) per thread
// with 16-byte loads, PR_INFLIGHT of them in flight per lane.  A CU pulls NP^2 / 2 * 8 B per walk at ~64 B per clock: 0.4 us at NP = 256, 1.7 us
// at 512 — against two passes of the eight-wave kernel at 25 GB/s per CU and against the 41-75 us of a six-launch lockstep round.
template <int KERNEL, bool WLDS>
__global__ __launch_bounds__(WLDS ? SEARCH_LDS_NP : SEARCH_MAX_NP) void polish_rows_kernel(const PolishFusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) double pr_smem[];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int sidx = (int)blockIdx.x;
  const int NP = a.NP, N = a.N, d = a.d, DP = a.DP;
  const int WLD = NP + 1;
  const PolishLds L = polish_lds(NP, d, DP, WLDS);
  double *Wl = pr_smem + L.W, *xs = pr_smem + L.xs, *ls_s = pr_smem + L.ls, *al_s = pr_smem + L.alpha, *ks = pr_smem + L.ks,
         *vs = pr_smem + L.vs, *cc = pr_smem + L.cc, *pp = pr_smem + L.pp, *us = pr_smem + L.us, *red = pr_smem + L.red,
         *opt = pr_smem + L.opt, *Xl = pr_smem + L.X;
  const int xs_staged = L.x_doubles;
  int* flag = (int*)(pr_smem + L.flag);
  const double* __restrict__ Xs = xs_staged ? Xl : a.Xs;
  const int xld = xs_staged ? DP + 1 : DP;

  if (WLDS) pr_load_w(Wl, a.W, NP, tid);
  al_s[tid] = a.alpha[tid];
  if (tid < 64) ls_s[tid] = (tid < d) ? a.ls[tid] : 1.0;
  if (xs_staged)
    for (int e = tid; e < NP * DP; e += NP) {
      const int k = e / DP, t = e - k * DP;
      Xl[k * (DP + 1) + t] = a.Xs[e];
    }
  RowsRun run{};
  if (wave == 0) {
    const bool mine = lane < d;
    run.lo = mine ? a.lo[lane] : 0.0;
    run.hi = mine ? a.hi[lane] : 0.0;
    run.xt = mine ? polish_min(polish_max(a.seeds[(size_t)sidx * d + lane], run.lo), run.hi) : 0.0;      // polish_start
    run.alpha = 1.0;
    run.status = 2;
    if (lane < DP) xs[lane] = mine ? run.xt / a.ls[lane] : 0.0;
    if (lane == 0) flag[0] = 0;
  }
  __syncthreads();

  // the sums over the training points: lane groups of DP lanes (one dimension each), group j takes the points k = j (mod groups)
  const int gpw = 64 / DP, groups = gpw * (NP >> 6);
  const int grp = wave * gpw + lane / DP, gt = lane % DP;
  const int round_cap = 4 * a.max_iter + 64;
  const double al_i = al_s[tid];
  const double* wrow = Wl + tid * WLD;

  for (int round = 0;; ++round) {
    // ---- k*_i and the gradient factor f_i of this thread's point
    double fi;
    {
      double d2;
      const double kv = pr_kstar<KERNEL>(xs, Xs + (int64_t)tid * xld, DP, d2);
      fi = gpbo_kernel_slope<KERNEL>(d2, kv);
      if (tid >= N) fi = 0.0;          // padding rows carry no gradient
      ks[tid] = kv;
    }
    __syncthreads();
    // ---- v = W k* and u = W^T v, then every point's two gradient weights and its terms of |v|^2 and k* . alpha
    if (WLDS) {
      // thread i: row i of W for v_i (zeros above the diagonal: the whole row), column i for u_i
      const double v = (tid < N) ? pr_row_lds(wrow, ks, NP) : 0.0;
      vs[tid] = v;
      pp[2 * tid] = v * v;
      pp[2 * tid + 1] = ks[tid] * al_i;
      __syncthreads();
      double u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
      const double* wcol = Wl + tid;
      for (int i = 0; i < NP; i += 4) {
        u0 = fma(wcol[i * WLD], vs[i], u0);
        u1 = fma(wcol[(i + 1) * WLD], vs[i + 1], u1);
        u2 = fma(wcol[(i + 2) * WLD], vs[i + 2], u2);
        u3 = fma(wcol[(i + 3) * WLD], vs[i + 3], u3);
      }
      cc[2 * tid] = al_i * fi;
      cc[2 * tid + 1] = ((u0 + u1) + (u2 + u3)) * fi;
    } else {
      // W in memory: the first NP / 2 threads walk TWO rows (columns) each with 16-byte loads — a wave instruction is 1 KB of one row
      // of Wt (of W) — wave w the rows 128 w .. 128 w + 127, whose columns end at 128 (w + 1) (the columns 128 w .., whose rows
      // start at 128 w): the zeros of the triangle are never loaded.  The sums come back through LDS to the points' own threads.
      typedef double d2 __attribute__((ext_vector_type(2)));
      const int ld2 = NP / 2;
      pr_rows_mem(a.Wt, ks, NP, N, tid, wave, vs);
      __syncthreads();
      pp[2 * tid] = vs[tid] * vs[tid];
      pp[2 * tid + 1] = ks[tid] * al_i;
      if (tid < ld2) {
        const d2* __restrict__ wc = reinterpret_cast<const d2*>(a.W) + tid;       // W[i][2 tid .. 2 tid + 1]
        double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
        for (int i = 128 * wave; i < NP; i += PR_INFLIGHT) {
          d2 w[PR_INFLIGHT];
#pragma unroll
          for (int e = 0; e < PR_INFLIGHT; ++e) w[e] = wc[(int64_t)(i + e) * ld2];
#pragma unroll
          for (int e = 0; e < PR_INFLIGHT; e += 2) {
            a0 = fma(w[e].x, vs[i + e], a0);
            b0 = fma(w[e].y, vs[i + e], b0);
            a1 = fma(w[e + 1].x, vs[i + e + 1], a1);
            b1 = fma(w[e + 1].y, vs[i + e + 1], b1);
          }
        }
        us[2 * tid] = a0 + a1;
        us[2 * tid + 1] = b0 + b1;
      }
      __syncthreads();
      cc[2 * tid] = al_i * fi;
      cc[2 * tid + 1] = us[tid] * fi;
    }
    __syncthreads();
    // ---- the sums over the points: gm_t = sum_k alpha_k f_k (x_t - X_kt), gv_t likewise with u_k; |v|^2 and k* . alpha ride along
    {
      const double xt = xs[gt];
      double gm = 0.0, gv = 0.0, s2 = 0.0, mm = 0.0;
      for (int k = grp; k < NP; k += groups) {
        const double df = xt - Xs[(int64_t)k * xld + gt];
        gm = fma(cc[2 * k], df, gm);
        gv = fma(cc[2 * k + 1], df, gv);
        s2 += pp[2 * k];
        mm += pp[2 * k + 1];
      }
      double* r = red + grp * (2 * DP + 2);
      r[gt] = gm;
      r[DP + gt] = gv;
      if (gt == 0) { r[2 * DP] = s2; r[2 * DP + 1] = mm; }
    }
    __syncthreads();
    // ---- wave 0, lane = variable: the groups in order, mean / deviation / acquisition, the optimiser's step
    if (wave == 0) {
      double sa = 0.0, sb = 0.0, tot0 = 0.0, tot1 = 0.0;
      const int t = lane < DP ? lane : 0;
      for (int j = 0; j < groups; ++j) {
        const double* r = red + j * (2 * DP + 2);
        sa += r[t];
        sb += r[DP + t];
        tot0 += r[2 * DP];
        tot1 += r[2 * DP + 1];
      }
      double var = fma(a.amplitude, 1.0 - tot0, a.white);
      if (var < 0.0) {
        if (lane == 0) *a.negvar = 1;
        var = 0.0;
      }
      const double sdn = sqrt(var);
      const double sd = sqrt(var * (a.y_std * a.y_std));
      const double mu = a.y_std * tot1 + a.y_mean;
      double dmu = 0.0, dsd = 0.0, g = 0.0;
      double av, ca, cs;
      polish_acq_coeffs(a.acq, a.acq_param, a.y_max, mu, sd, DevCdf(), DevPdf(), DevErfcx(), av, ca, cs);
      if (lane < d) {
        const double inv_l = 1.0 / ls_s[lane];
        dmu = a.y_std * sa * inv_l;
        dsd = (sdn > 0.0) ? -((a.y_std * sb * inv_l) * a.amplitude) / sdn : 0.0;       // a clipped (zero) variance has no slope
        g = polish_acq_grad(ca, cs, dmu, dsd);
        if (!__builtin_isfinite(g)) g = 0.0;
      }
      if (a.eval_only) {
        if (round + 1 >= a.eval_only) {
          double* o = a.dbg + (size_t)sidx * (4 + 3 * d);
          if (lane == 0) { o[0] = -av; o[1] = mu; o[2] = sd; o[3] = 0.0; }
          if (lane < d) { o[4 + lane] = g; o[4 + d + lane] = dmu; o[4 + 2 * d + lane] = dsd; }
          if (lane == 0) flag[0] = 1;
        }
      } else {
        pr_advance(run, -av, g, d, lane, opt, a.max_iter);
        if (lane < DP) xs[lane] = (lane < d) ? run.xt / ls_s[lane] : 0.0;
        if (lane == 0) flag[0] = (run.phase == 2 || round + 1 > round_cap) ? 1 : 0;
      }
    }
    __syncthreads();
    if (flag[0]) break;
  }
  if (a.eval_only) return;
  if (wave == 0) {
    if (lane < d) a.x_out[(size_t)sidx * d + lane] = run.x;
    if (lane == 0) {
      a.f_out[sidx] = run.f;
      a.status_out[sidx] = run.phase == 2 ? run.status : 2;
      a.iter_out[sidx] = run.iter;
      a.eval_out[sidx] = run.evals;
    }
  }
}

}  // namespace

int ensure_w_transposed(gpbo_ctx* ctx, Model& m) {
  if (!m.wt_valid) {
    transpose_w_kernel<<<dim3((unsigned)(m.NP / 64), (unsigned)(m.NP / 64)), dim3(256), 0, ctx->stream>>>(m.W, m.K, (int)m.NP);
    GPBO_HIP(ctx, hipGetLastError());
    m.wt_valid = true;
  }
  return GPBO_OK;
}

int launch_polish_fused(gpbo_ctx* ctx, Model& m, const PolishPlan& plan, const PolishBlock& block, int acq, double acq_param,
                        double y_max, double y_mean, double y_std, const double* seeds, int n_seeds, const double* box_lo,
                        const double* box_hi, int max_iter, int eval_repeat) {
  if (plan.mode == SearchMode::NotServed) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "launch_polish_fused: the model is outside the one-launch path's range");
  const int d = m.d;
  if (!(ctx->func_attrs & ATTR_POLISH_FUSED)) {
    const int rc = for_each_kernel_wlds(ctx, [&](auto k, auto wlds) -> int {
      GPBO_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(polish_rows_kernel<decltype(k)::value, decltype(wlds)::value>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, SEARCH_LDS_BYTES));
      return GPBO_OK;
    });
    if (rc) return rc;
    ctx->func_attrs |= ATTR_POLISH_FUSED;
  }
  double* h = (double*)ctx->polish_pinned;
  std::copy(seeds, seeds + (size_t)n_seeds * d, h + block.seeds);
  std::copy(box_lo, box_lo + d, h + block.lo);
  std::copy(box_hi, box_hi + d, h + block.hi);
  PolishFusedArgs a{};
  a.W = m.W; a.Xs = m.Xs; a.alpha = m.alpha; a.ls = m.ls;
  a.NP = (int)m.NP; a.N = (int)m.N; a.d = d; a.DP = m.DP;
  a.y_mean = y_mean; a.y_std = y_std;
  a.amplitude = m.amplitude; a.white = m.white;
  a.acq = acq; a.acq_param = acq_param; a.y_max = y_max;
  a.max_iter = max_iter; a.eval_only = eval_repeat;
  double* dv = (double*)ctx->polish_pinned_dev;
  int* iv = (int*)dv;
  a.seeds = dv + block.seeds; a.lo = dv + block.lo; a.hi = dv + block.hi;
  a.x_out = dv + block.x; a.f_out = dv + block.f; a.dbg = dv + block.dbg;
  a.status_out = iv + block.status; a.iter_out = iv + block.iter; a.eval_out = iv + block.evals;
  a.negvar = ctx->negvar;
  if (plan.mode == SearchMode::WInMemory) {
    // the transposed copy for the row walk lives in the slot's K buffer (a fit assembles K straight into L; gpbo_get_K and the LML
    // path, which write K, invalidate it): made once per fit
    if (const int rc = ensure_w_transposed(ctx, m)) return rc;
    a.Wt = m.K;
  }
  if (const int rc = with_kernel_wlds(ctx, m.kernel, plan.mode == SearchMode::WInLds, [&](auto k, auto wlds) -> int {
    polish_rows_kernel<decltype(k)::value, decltype(wlds)::value><<<dim3((unsigned)n_seeds), dim3((unsigned)m.NP), (size_t)plan.lds_bytes, ctx->stream>>>(a);
    return GPBO_OK;
  })) return rc;
  GPBO_HIP(ctx, hipGetLastError());
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GPBO_OK;
}

}  // namespace gpbo
