// gpbo_qnei_greedy (gfx950): a batch of q candidates by greedy noisy expected improvement over T joint posterior draws
// (include/gpbo.h has the formulas and the conventions; qnei_plan.h the workspace and the score kernel's thread rule).
//
// The draws' values are made by the kernels of gpbo_sample_paths (posterior_paths.hip: launch_path_weights, then path_eval_kernel
// through launch_paths_over) — per group over the candidates into rows [g S, (g + 1) S) of a resident (T, M) block, and over the
// training and the pending points into a small [T][N + P] buffer.  New here:
//   qnei_baseline_kernel   a wave per draw: m_t = the fmax fold of the draw's row of that buffer (or of y_best and its pending part)
//   qnei_score_kernel      the hot loop, once per greedy step: thread = one or two candidates (qnei_items), walking the T rows of
//                          the block — consecutive lanes read consecutive 8 or 16 bytes of a row — with the m_t staged in LDS and read
//                          back as broadcasts.  Per value one subtract, one compare / select and one add; the kernel is the stream of
//                          the block's 8 T M bytes.  It applies the picked mask and writes key_j into ctx->ys
//   qnei_update_kernel     one workgroup behind the step's selection: reads the pick from the selection's device record (the first
//                          NaN wins, as best_of_selection has it), files {gain, index}, marks the mask, and folds column `pick` of
//                          the block into the m_t
// No multiply-add in any of them (the file is compiled with -ffp-contract=off as well): tests replay the keys bit for bit.
//
// gpbo_cnei_greedy (the constrained form; cnei_plan.h has its workspace) lives here too, because it runs the same kernels — a kernel
// cannot be launched from another translation unit.  Its block holds the MASKED objective draws (path_plan.h: PATH_MASKED: -inf where
// the constraint draws call a point infeasible), which the baseline and the score kernel take as they are: -inf - m_t is not > 0
// and fmax(m_t, -inf) = m_t.  New for it:
//   cnei_update_kernel     qnei_update_kernel's work (the one device function both call) plus the share of draws that call the
//                          pick feasible, in a record {gain, index, feasible} of its own
#include "greedy.h"

#include <cmath>
#include <limits>

namespace gpbo {

struct CneiRecord { double gain; int64_t idx; double feasible; };      // gpbo_cnei_greedy's (greedy_fetch checks its room)
static_assert(sizeof(CneiRecord) == 24, "a record is three doubles of the workspace");

// m[t] = m0[t] = fmax fold of (y_best unless noisy) and base[t][c0 .. ldb): lane l takes c0 + l, c0 + l + 64, ..., the 64 partial
// maxima meet in a butterfly.  fmax drops a NaN operand and orders numbers totally up to a zero's sign, so the fold's value is the
// index-order fold's.
__global__ __launch_bounds__(64) void qnei_baseline_kernel(const double* __restrict__ base, int64_t ldb, int c0, int noisy, double y_best,
                                                           double* __restrict__ m, double* __restrict__ m0) {
  const int t = blockIdx.x, lane = threadIdx.x;
  const double* row = base + (int64_t)t * ldb;
  double acc = std::numeric_limits<double>::quiet_NaN();
  for (int64_t c = c0 + lane; c < ldb; c += 64) acc = fmax(acc, row[c]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc = fmax(acc, __shfl_xor(acc, off));
  if (!noisy) acc = fmax(y_best, acc);
  if (lane == 0) { m[t] = acc; m0[t] = acc; }
}

// term_t = f - m_t where that is > 0, 0 where it is not, NaN for a NaN f
__device__ __forceinline__ double qnei_term(double f, double mt) {
  const double d = f - mt;
  return d > 0.0 ? d : (f != f ? f : 0.0);
}

// key_j over the candidates: ITEMS (qnei_plan.h: qnei_items) neighbouring candidates per thread, read as one load per row
template <int ITEMS>
__global__ __launch_bounds__(QNEI_BLOCK) void qnei_score_kernel(const double* __restrict__ vals, int64_t M, int T,
                                                                const double* __restrict__ m, const uint8_t* __restrict__ mask,
                                                                double* __restrict__ ys) {
  __shared__ double ms[QNEI_MAX_DRAWS];
  for (int t = threadIdx.x; t < T; t += QNEI_BLOCK) ms[t] = m[t];
  __syncthreads();
  const int64_t i = qnei_first_candidate(blockIdx.x, threadIdx.x, ITEMS);
  if (i >= M) return;
  const double inf = std::numeric_limits<double>::infinity();
  const double* col = vals + i;
  if (ITEMS == 2) {      // M is even: i + 1 < M, and every row's pair sits on a 16-byte boundary
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (int t = 0; t < T; ++t) {
      const double2 f = *reinterpret_cast<const double2*>(col + (int64_t)t * M);
      const double mt = ms[t];
      s0 += qnei_term(f.x, mt);
      s1 += qnei_term(f.y, mt);
    }
    const uchar2 picked = *reinterpret_cast<const uchar2*>(mask + i);
    double2 key;
    key.x = picked.x ? inf : -(s0 / (double)T);
    key.y = picked.y ? inf : -(s1 / (double)T);
    *reinterpret_cast<double2*>(ys + i) = key;
  } else {
    double s0 = 0.0;
#pragma unroll 8
    for (int t = 0; t < T; ++t) s0 += qnei_term(col[(int64_t)t * M], ms[t]);
    ys[i] = mask[i] ? inf : -(s0 / (double)T);
  }
}

// Behind step j's selection, for both update kernels: the pick (greedy_pick) marked in the mask and absorbed into the incumbents
__device__ __forceinline__ GreedyPick qnei_absorb_pick(const SelState* __restrict__ st, const Key* __restrict__ first,
                                                       const double* __restrict__ vals, int64_t M, int T, int64_t offset,
                                                       double* __restrict__ m, uint8_t* __restrict__ mask) {
  const GreedyPick p = greedy_pick(st, first, M, offset);
  if (p.local < 0) return p;
  if (threadIdx.x == 0) mask[p.local] = 1;
  for (int t = threadIdx.x; t < T; t += QNEI_BLOCK) m[t] = fmax(m[t], vals[(int64_t)t * M + p.local]);
  return p;
}

__global__ __launch_bounds__(QNEI_BLOCK) void qnei_update_kernel(const SelState* __restrict__ st, const Key* __restrict__ first,
                                                                 const double* __restrict__ vals, int64_t M, int T, int64_t offset, int j,
                                                                 double* __restrict__ m, uint8_t* __restrict__ mask,
                                                                 GreedyRecord* __restrict__ rec) {
  const GreedyPick p = qnei_absorb_pick(st, first, vals, M, T, offset, m, mask);
  if (threadIdx.x == 0) rec[j] = GreedyRecord{p.gain, p.idx};
}

// ... and, over the masked block, feasible = (the number of draws t whose value at the pick is > -inf) / T: NaN for a NaN pick
__global__ __launch_bounds__(QNEI_BLOCK) void cnei_update_kernel(const SelState* __restrict__ st, const Key* __restrict__ first,
                                                                 const double* __restrict__ vals, int64_t M, int T, int64_t offset, int j,
                                                                 double* __restrict__ m, uint8_t* __restrict__ mask,
                                                                 CneiRecord* __restrict__ rec) {
  __shared__ int count;
  if (threadIdx.x == 0) count = 0;
  __syncthreads();
  const GreedyPick p = qnei_absorb_pick(st, first, vals, M, T, offset, m, mask);
  if (p.local >= 0) {
    int mine = 0;
    for (int t = threadIdx.x; t < T; t += QNEI_BLOCK) mine += vals[(int64_t)t * M + p.local] > -std::numeric_limits<double>::infinity();
    if (mine) atomicAdd(&count, mine);
  }
  __syncthreads();
  if (threadIdx.x == 0)
    rec[j] = CneiRecord{p.gain, p.idx, (p.nan || p.local < 0) ? std::numeric_limits<double>::quiet_NaN() : (double)count / (double)T};
}

// The q greedy steps of both entry points (greedy_steps) over the block `vals`; `update(st, first, j)` launches the caller's update kernel
template <class Update>
static int qnei_steps(gpbo_ctx* ctx, const double* vals, int64_t M, int T, const double* mt, const uint8_t* mask, int q,
                      double* keys_out, Update update) {
  const int items = qnei_items(M);
  const dim3 grid((unsigned)qnei_score_blocks(M)), block(QNEI_BLOCK);
  return greedy_steps(ctx, M, q, keys_out, [&] {
    if (items == 2) qnei_score_kernel<2><<<grid, block, 0, ctx->stream>>>(vals, M, T, mt, mask, ctx->ys);
    else qnei_score_kernel<1><<<grid, block, 0, ctx->stream>>>(vals, M, T, mt, mask, ctx->ys);
  }, update);
}

int launch_qnei_greedy(gpbo_ctx* ctx, const Model& m, int64_t M, double y_mean, double y_std, int G, int S, int F, const double* omega,
                       const double* phase, const double* weights, const double* eps, int noisy, double y_best, const double* pending,
                       int P, int q, int64_t index_offset, int64_t* pick_idx, double* pick_gain, double* baseline_out,
                       double* values_out, double* keys_out) {
  int rc;
  const int N = (int)m.N, d = m.d, T = G * S;
  const QneiBlock b = qnei_block(T, M, N, P, d, m.DP, q);
  if ((rc = ensure(ctx, &ctx->greedy, &ctx->cap_greedy, b.doubles))) return rc;
  double* w = ctx->greedy;
  double *vals = w + b.vals, *base = w + b.base, *mt = w + b.m, *pend_s = w + b.pend_s;
  uint8_t* mask = (uint8_t*)(w + b.mask);
  GreedyRecord* rec = (GreedyRecord*)(w + b.rec);
  // the scaled candidates (the draws' workspace of the context, as gpbo_sample_paths fills it) and the scaled pending points
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * m.DP))) return rc;
  greedy_mark(ctx, ctx->qnei_clock, 0);
  if ((rc = launch_prescale(ctx, ctx->Xc, M, d, m.DP, m.ls, ctx->Xcs, Mp))) return rc;
  if (P > 0) {
    GPBO_HIP(ctx, hipMemcpyAsync(w + b.pend, pending, (size_t)P * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_prescale(ctx, w + b.pend, P, d, m.DP, m.ls, pend_s, P))) return rc;
  }
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  GPBO_HIP(ctx, hipMemsetAsync(mask, 0, (size_t)((M + 7) / 8 * 8), ctx->stream));
  // the draws, group by group: the group's inputs and path weights into the paths workspace, then its S rows of each buffer
  const Model* one = &m;
  const GreedyDraws draws = greedy_draws(1, &one, G, S, F, omega, phase, weights, eps);
  for (int g = 0; g < G; ++g) {
    PathWorkspace ws{};
    if ((rc = greedy_path_weights(ctx, draws, m, 0, g, &ws))) return rc;
    if ((rc = launch_paths_over(ctx, m, ws, y_mean, y_std, S, F, ctx->Xcs, M, vals + (int64_t)g * S * M, M))) return rc;
    double* rows = base + (int64_t)g * S * b.ldb;
    if (noisy && (rc = launch_paths_over(ctx, m, ws, y_mean, y_std, S, F, m.Xs, N, rows, b.ldb))) return rc;
    if (P > 0 && (rc = launch_paths_over(ctx, m, ws, y_mean, y_std, S, F, pend_s, P, rows + N, b.ldb))) return rc;
  }
  qnei_baseline_kernel<<<dim3((unsigned)T), dim3(64), 0, ctx->stream>>>(base, b.ldb, noisy ? 0 : N, noisy, y_best, mt, w + b.m0);
  GPBO_HIP(ctx, hipGetLastError());
  greedy_mark(ctx, ctx->qnei_clock, 1);
  if ((rc = qnei_steps(ctx, vals, M, T, mt, mask, q, keys_out, [&](const SelState* st, const Key* first, int j) {
        qnei_update_kernel<<<dim3(1), dim3(QNEI_BLOCK), 0, ctx->stream>>>(st, first, vals, M, T, index_offset, j, mt, mask, rec);
      })))
    return rc;
  greedy_mark(ctx, ctx->qnei_clock, 2);
  const GreedyRecord* hrec;
  if ((rc = greedy_fetch(ctx, rec, q, &hrec))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(baseline_out, w + b.m0, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (values_out)
    GPBO_HIP(ctx, hipMemcpyAsync(values_out, vals, (size_t)T * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int j = 0; j < q; ++j) { pick_idx[j] = hrec[j].idx; pick_gain[j] = hrec[j].gain; }
  return GPBO_OK;
}

// gpbo_cnei_greedy behind its argument checks: ms / y_mean / y_std per slot (the objective, then the C constraints), the draws'
// inputs concatenated slot-major, then group-major.
int launch_cnei_greedy(gpbo_ctx* ctx, int C, const Model* const* ms, int64_t M, const double* y_mean, const double* y_std,
                       const double* lb, const double* ub, int G, int S, int F, const double* omega, const double* phase,
                       const double* weights, const double* eps, double y_floor, const double* base_pts, int B, int q,
                       int64_t index_offset, int64_t* pick_idx, double* pick_gain, double* pick_feasible, double* baseline_out,
                       double* values_out, double* viol_out, double* base_values_out, double* keys_out) {
  int rc;
  const int d = ms[0]->d, DP = ms[0]->DP, T = G * S;
  const CneiBlock b = cnei_block(T, S, M, B, d, DP, q, values_out != nullptr, base_values_out != nullptr && B > 0);
  if ((rc = ensure(ctx, &ctx->greedy, &ctx->cap_greedy, b.doubles))) return rc;
  double* w = ctx->greedy;
  double *vals = w + b.vals, *base = w + b.base, *mt = w + b.m, *viol = w + b.viol, *violb = w + b.violb, *pts_s = w + b.pts_s;
  double* stage = values_out ? w + b.stage : nullptr;
  double* stageb = (base_values_out && B > 0) ? w + b.stageb : nullptr;
  uint8_t* mask = (uint8_t*)(w + b.mask);
  CneiRecord* rec = (CneiRecord*)(w + b.rec);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  greedy_mark(ctx, ctx->cnei_clock, 0);
  GPBO_HIP(ctx, hipMemsetAsync(mask, 0, (size_t)((M + 7) / 8 * 8), ctx->stream));
  if (B > 0) GPBO_HIP(ctx, hipMemcpyAsync(w + b.pts, base_pts, (size_t)B * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const GreedyDraws draws = greedy_draws(C + 1, ms, G, S, F, omega, phase, weights, eps);
  // the draws, group by group; per group the constraints in slot order (the violation's sum order), the objective last: per slot
  // the group's path weights, the candidates and the base points scaled by THAT slot's length scales, one pass over each
  const size_t cand_bytes = (size_t)S * (size_t)M * sizeof(double), base_bytes = (size_t)S * (size_t)B * sizeof(double);
  for (int g = 0; g < G; ++g) {
    const int64_t row = (int64_t)g * S;
    for (int k = 1; k <= C + 1; ++k) {
      const int j = k <= C ? k : 0;
      const Model& m = *ms[j];
      PathWorkspace ws{};
      if ((rc = greedy_path_weights(ctx, draws, m, j, g, &ws))) return rc;
      if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
      const int epilogue = j == 0 ? (int)PATH_MASKED : path_epilogue(j);
      const double lo = j ? lb[j - 1] : 0.0, hi = j ? ub[j - 1] : 0.0;
      if ((rc = launch_paths_over_fold(ctx, m, ws, y_mean[j], y_std[j], S, F, ctx->Xcs, M, j ? nullptr : vals + row * M, M,
                                       PathFold{epilogue, lo, hi, viol, stage})))
        return rc;
      if (values_out)      // stream order: the next pass overwrites the stage after this copy has read it
        GPBO_HIP(ctx, hipMemcpyAsync(values_out + ((int64_t)j * T + row) * M, stage, cand_bytes, hipMemcpyDeviceToHost, ctx->stream));
      if (B > 0) {
        if ((rc = launch_prescale(ctx, w + b.pts, B, d, DP, m.ls, pts_s, B))) return rc;
        if ((rc = launch_paths_over_fold(ctx, m, ws, y_mean[j], y_std[j], S, F, pts_s, B, j ? nullptr : base + row * b.ldb, b.ldb,
                                         PathFold{epilogue, lo, hi, violb, stageb})))
          return rc;
        if (stageb)
          GPBO_HIP(ctx, hipMemcpyAsync(base_values_out + ((int64_t)j * T + row) * B, stageb, base_bytes, hipMemcpyDeviceToHost,
                                       ctx->stream));
      }
    }
    if (viol_out) GPBO_HIP(ctx, hipMemcpyAsync(viol_out + row * M, viol, cand_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  qnei_baseline_kernel<<<dim3((unsigned)T), dim3(64), 0, ctx->stream>>>(base, b.ldb, 0, 0, y_floor, mt, w + b.m0);
  GPBO_HIP(ctx, hipGetLastError());
  greedy_mark(ctx, ctx->cnei_clock, 1);
  if ((rc = qnei_steps(ctx, vals, M, T, mt, mask, q, keys_out, [&](const SelState* st, const Key* first, int j) {
        cnei_update_kernel<<<dim3(1), dim3(QNEI_BLOCK), 0, ctx->stream>>>(st, first, vals, M, T, index_offset, j, mt, mask, rec);
      })))
    return rc;
  greedy_mark(ctx, ctx->cnei_clock, 2);
  const CneiRecord* hrec;
  if ((rc = greedy_fetch(ctx, rec, q, &hrec))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(baseline_out, w + b.m0, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int j = 0; j < q; ++j) { pick_idx[j] = hrec[j].idx; pick_gain[j] = hrec[j].gain; pick_feasible[j] = hrec[j].feasible; }
  return GPBO_OK;
}

}  // namespace gpbo
