// gpbo_qnhvi_greedy (gfx950): a batch of q candidates by greedy noisy expected hypervolume improvement over T joint posterior
// draws of m = 2 objectives (Daulton, Balandat & Bakshy 2021; include/gpbo.h has the formulas and the conventions; qnehvi_plan.h the
// workspace, the score kernel's thread rule and the LDS stage).
//
// The draws' values are made by the kernels of gpbo_sample_paths (posterior_paths.hip: launch_path_weights, then path_eval_kernel
// through launch_paths_over), slot by slot and group by group, over the candidates into rows [g S, (g + 1) S) of objective j's
// (T, M) block and over the slot-scaled base points into a small [2][T][B] buffer — as qnei.hip has them for one objective.  New here:
//   qnehvi_front_kernel    a workgroup per draw: the draw's front from its B value pairs, point by point from the right.  Point
//                          k + 1 is the lexicographic maximum (objective 0, then objective 1) of the pairs above ref_0 whose
//                          objective 1 exceeds point k's (ref_1 for the first): no pair with a larger objective 0 is left above that
//                          floor, so it is not dominated, and its objective 0 is strictly below point k's.  One block-wide arg-max
//                          per point; duplicates, ties and NaNs fall out of the comparisons.  O(B n) for a front of n points
//   qnehvi_score_kernel    the hot loop, once per greedy step: thread = one or two candidates (qnei_items), walking the T rows of
//                          both blocks — consecutive lanes read consecutive 8 or 16 bytes of a row, four draws' loads in flight —,
//                          the fronts staged in LDS as strips (a_{k+1}, c_k), QNEHVI_CHUNK draws at a time, and read back as
//                          wave-wide 16-byte broadcasts with a_k carried in a register.  It applies the picked mask and writes key_j
//                          into ctx->ys
//   qnehvi_update_kernel   one workgroup behind the step's selection: reads the pick from the selection's device record (the first
//                          NaN wins), files {gain, index}, marks the mask, and thread t inserts column `pick` of the blocks into
//                          draw t's front (qnehvi_insert)
// No multiply-add in any of them (the file is compiled with -ffp-contract=off as well): tests replay the keys bit for bit.
//
// gpmo_cnhvi_greedy (the constrained form; include/gpmo.h has the rule, cmo_plan.h its workspace) lives here too, because it runs
// the same front and score kernels — a kernel cannot be launched from another translation unit.  Its block holds objective 0's MASKED
// draws (path_plan.h: PATH_MASKED: -inf where the draw's constraint draws call a point infeasible) and objective 1's raw ones, which
// the three rules above take as they are: `x > ref0` fails for -inf (front build, insertion), and min(-inf, a_k) - a_{k+1} is not
// > 0, so every strip's width is 0 and 0 h = +0 for the finite h.  New for it:
//   cnhvi_update_kernel    qnehvi_update_kernel's work plus the share of draws that call the pick feasible, in a record
//                          {gain, index, feasible} of its own
#include "greedy.h"
#include "qnehvi_plan.h"
#include "cmo_plan.h"

#include <cmath>
#include <limits>
#include <string>

namespace gpbo {

static_assert(QNEI_MAX_DRAWS <= QNEI_BLOCK, "qnehvi_update_kernel gives every draw a thread of its one workgroup");

// (a, c) < (oa, oc) in the lexicographic order of the front's arg-max
__device__ __forceinline__ bool qnehvi_less(double a, double c, double oa, double oc) { return oa > a || (oa == a && oc > c); }

// The front of draw t = blockIdx.x from the pairs (v0[t ld + i], v1[t ld + i]), i < n: front[t][k] its points by objective 0
// descending, size[t] their number (both twice: the live copy and the one gpbo_qnhvi_greedy hands back as "before the first
// pick").  A front of more than QNEHVI_FRONT points raises the flag (T - t: the lowest draw stays) and is cut at QNEHVI_FRONT, so
// that what runs behind it stays inside its arrays.
__global__ __launch_bounds__(QNEI_BLOCK) void qnehvi_front_kernel(const double* __restrict__ v0, const double* __restrict__ v1,
                                                                  int64_t ld, int n, double ref0, double ref1, int T,
                                                                  double2* __restrict__ front, double2* __restrict__ front0,
                                                                  int* __restrict__ size, int* __restrict__ size0,
                                                                  int* __restrict__ flag) {
  __shared__ double wa[QNEI_BLOCK / 64], wc[QNEI_BLOCK / 64];
  __shared__ double best[2];
  const int t = blockIdx.x, tid = threadIdx.x;
  const double* r0 = v0 + (int64_t)t * ld;
  const double* r1 = v1 + (int64_t)t * ld;
  const double none = -std::numeric_limits<double>::infinity();      // ref0 is finite: every admitted pair is above it
  double floor_c = ref1;
  int count = 0;
  for (;;) {
    double a = none, c = none;
    for (int i = tid; i < n; i += QNEI_BLOCK) {
      const double x = r0[i], y = r1[i];
      if (x > ref0 && y > floor_c && qnehvi_less(a, c, x, y)) { a = x; c = y; }      // a NaN fails a comparison
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double oa = __shfl_xor(a, off), oc = __shfl_xor(c, off);
      if (qnehvi_less(a, c, oa, oc)) { a = oa; c = oc; }
    }
    if ((tid & 63) == 0) { wa[tid >> 6] = a; wc[tid >> 6] = c; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < QNEI_BLOCK / 64; ++w)
        if (qnehvi_less(a, c, wa[w], wc[w])) { a = wa[w]; c = wc[w]; }
      best[0] = a; best[1] = c;
    }
    __syncthreads();
    a = best[0]; c = best[1];
    if (a == none) break;
    if (count == QNEHVI_FRONT) {
      if (tid == 0) atomicMax(flag, T - t);
      break;
    }
    if (tid == 0) {
      const double2 p = make_double2(a, c);
      front[(int64_t)t * QNEHVI_FRONT + count] = p;
      front0[(int64_t)t * QNEHVI_FRONT + count] = p;
    }
    ++count;
    floor_c = c;
  }
  if (tid == 0) { size[t] = count; size0[t] = count; }
}

// The update rule of one front f[0 .. *n) (objective 0 descending, objective 1 ascending) for y = (y0, y1): unchanged if y has a NaN,
// is not strictly above ref in both, or is dominated by or equal to a point; else the points y dominates — a run, since objective 1
// ascends — leave and y takes their place.  true: the front would outgrow QNEHVI_FRONT (it is left as it is).
__device__ inline bool qnehvi_insert(double2* __restrict__ f, int* __restrict__ n_p, double y0, double y1, double ref0, double ref1) {
  if (!(y0 > ref0 && y1 > ref1)) return false;
  const int n = *n_p;
  int p = 0;
  while (p < n && f[p].x > y0) ++p;                      // [0, p): strictly to the right of y; the last of them is their highest
  if (p > 0 && f[p - 1].y >= y1) return false;
  if (p < n && f[p].x == y0 && f[p].y >= y1) return false;
  int r = p;
  while (r < n && f[r].y <= y1) ++r;                     // [p, r): not to the right of y and not above it
  const int gone = r - p;
  if (n - gone + 1 > QNEHVI_FRONT) return true;
  if (gone == 0) {
    for (int k = n - 1; k >= p; --k) f[k + 1] = f[k];
  } else if (gone > 1) {
    for (int k = r; k < n; ++k) f[k - gone + 1] = f[k];
  }
  f[p] = make_double2(y0, y1);
  *n_p = n - gone + 1;
  return false;
}

// w_k h_k of one strip: one rounded product of two clamped differences
__device__ __forceinline__ double qnehvi_term(double f0, double f1, double a_k, double a_next, double c_k) {
  const double w = (f0 < a_k ? f0 : a_k) - a_next;
  const double h = f1 - c_k;
  return (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
}

constexpr int QNEHVI_AHEAD = 4;      // draws whose rows a thread has in flight before it walks their strips

// key_j over the candidates: ITEMS (qnei_plan.h: qnei_items) neighbouring candidates per thread, read as one load per row and objective
template <int ITEMS>
__global__ __launch_bounds__(QNEI_BLOCK) void qnehvi_score_kernel(const double* __restrict__ vals, int64_t M, int T,
                                                                  const double2* __restrict__ front, const int* __restrict__ size,
                                                                  double ref0, double ref1, const uint8_t* __restrict__ mask,
                                                                  double* __restrict__ ys) {
  __shared__ double2 strips[QNEHVI_CHUNK * QNEHVI_STRIPS];
  __shared__ int ns[QNEHVI_CHUNK];
  static_assert(sizeof(strips) + sizeof(ns) == QNEHVI_LDS_BYTES, "qnehvi_plan.h states the stage's size");
  const int64_t i = qnei_first_candidate(blockIdx.x, threadIdx.x, ITEMS);
  const bool live = i < M;      // (with ITEMS == 2 M is even: i + 1 < M too, and every row's pair sits on a 16-byte boundary)
  const double* col0 = vals + (live ? i : 0);
  const double* col1 = col0 + (int64_t)T * M;
  const double inf = std::numeric_limits<double>::infinity();
  double s[ITEMS];
#pragma unroll
  for (int c = 0; c < ITEMS; ++c) s[c] = 0.0;
  for (int t0 = 0; t0 < T; t0 += QNEHVI_CHUNK) {
    const int C = T - t0 < QNEHVI_CHUNK ? T - t0 : QNEHVI_CHUNK;
    __syncthreads();      // the stage before this one has been read
    for (int e = threadIdx.x; e < C * QNEHVI_STRIPS; e += QNEI_BLOCK) {
      const int tl = e / QNEHVI_STRIPS, k = e - tl * QNEHVI_STRIPS;
      const int n = size[t0 + tl];
      if (k <= n) {      // strip k = (a_{k+1}, c_k), a_{n+1} = ref0, c_0 = ref1
        const double2* f = front + (int64_t)(t0 + tl) * QNEHVI_FRONT;
        strips[e] = make_double2(k < n ? f[k].x : ref0, k > 0 ? f[k - 1].y : ref1);
      }
      if (k == 0) ns[tl] = n;
    }
    __syncthreads();
    if (!live) continue;
    for (int tl = 0; tl < C; tl += QNEHVI_AHEAD) {
      double f0[QNEHVI_AHEAD][ITEMS], f1[QNEHVI_AHEAD][ITEMS];
#pragma unroll
      for (int u = 0; u < QNEHVI_AHEAD; ++u) {
        const int64_t row = (int64_t)(t0 + (tl + u < C ? tl + u : C - 1)) * M;      // (past the chunk: its last row again, unused)
        if (ITEMS == 2) {
          const double2 x = *reinterpret_cast<const double2*>(col0 + row), y = *reinterpret_cast<const double2*>(col1 + row);
          f0[u][0] = x.x; f0[u][ITEMS - 1] = x.y; f1[u][0] = y.x; f1[u][ITEMS - 1] = y.y;
        } else {
          f0[u][0] = col0[row]; f1[u][0] = col1[row];
        }
      }
#pragma unroll
      for (int u = 0; u < QNEHVI_AHEAD; ++u) {
        if (tl + u >= C) break;
        const int n = ns[tl + u];
        const double2* sp = strips + (tl + u) * QNEHVI_STRIPS;
        double hvi[ITEMS];
#pragma unroll
        for (int c = 0; c < ITEMS; ++c) hvi[c] = 0.0;
        double a_k = inf;
        for (int k = 0; k <= n; ++k) {
          const double2 st = sp[k];
#pragma unroll
          for (int c = 0; c < ITEMS; ++c) hvi[c] += qnehvi_term(f0[u][c], f1[u][c], a_k, st.x, st.y);
          a_k = st.x;
        }
#pragma unroll
        for (int c = 0; c < ITEMS; ++c) {
          const double x = f0[u][c], y = f1[u][c];
          s[c] += (x != x || y != y) ? std::numeric_limits<double>::quiet_NaN() : hvi[c];
        }
      }
    }
  }
  if (!live) return;
  if (ITEMS == 2) {
    const uchar2 picked = *reinterpret_cast<const uchar2*>(mask + i);
    double2 key;
    key.x = picked.x ? inf : -(s[0] / (double)T);
    key.y = picked.y ? inf : -(s[ITEMS - 1] / (double)T);
    *reinterpret_cast<double2*>(ys + i) = key;
  } else {
    ys[i] = mask[i] ? inf : -(s[0] / (double)T);
  }
}

// Behind step j's selection: the pick (greedy_pick), its record, the mask, the fronts.
__global__ __launch_bounds__(QNEI_BLOCK) void qnehvi_update_kernel(const SelState* __restrict__ st, const Key* __restrict__ first,
                                                                   const double* __restrict__ vals, int64_t M, int T, int64_t offset,
                                                                   int j, double ref0, double ref1, double2* __restrict__ front,
                                                                   int* __restrict__ size, uint8_t* __restrict__ mask,
                                                                   GreedyRecord* __restrict__ rec, int* __restrict__ flag) {
  const GreedyPick p = greedy_pick(st, first, M, offset);
  const int64_t pick = p.local;
  const int t = threadIdx.x;
  if (t == 0) {
    rec[j] = GreedyRecord{p.gain, p.idx};
    if (pick >= 0) mask[pick] = 1;
  }
  if (pick < 0 || t >= T) return;
  const double y0 = vals[(int64_t)t * M + pick], y1 = vals[((int64_t)T + t) * M + pick];
  if (qnehvi_insert(front + (int64_t)t * QNEHVI_FRONT, size + t, y0, y1, ref0, ref1)) atomicMax(flag, T - t);
}

// the refusal behind the call's one synchronisation: flag = T - t for the lowest draw t whose front outgrew its array
static int qnehvi_overflow(gpbo_ctx* ctx, const char* who, int T, int flag) {
  GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, std::string(who) + ": the front of draw " + std::to_string(T - flag) + " outgrew " +
                                           std::to_string(QNEHVI_FRONT) + " points (GPBO_MAX_QNEHVI_FRONT); a front is never thinned");
}

#ifdef GPBO_DEBUG
// the insertion rule on given values: thread t inserts (ins[t ld + i], ins[(T + t) ld + i]), i = 0 .. n_insert - 1 in order
__global__ __launch_bounds__(QNEI_BLOCK) void qnehvi_insert_kernel(const double* __restrict__ ins, int64_t ld, int n_insert, int T,
                                                                   double ref0, double ref1, double2* __restrict__ front,
                                                                   int* __restrict__ size, int* __restrict__ flag) {
  const int t = blockIdx.x * QNEI_BLOCK + threadIdx.x;
  if (t >= T) return;
  for (int i = 0; i < n_insert; ++i)
    if (qnehvi_insert(front + (int64_t)t * QNEHVI_FRONT, size + t, ins[(int64_t)t * ld + i], ins[((int64_t)T + t) * ld + i], ref0, ref1))
      atomicMax(flag, T - t);
}

int debug_qnehvi_fronts(gpbo_ctx* ctx, int T, int n, const double* base_values, const double* ref, int n_insert,
                        const double* insert_values, int* front_size_out, double* fronts_out) {
  int rc;
  const QnehviBlock b = qnehvi_block(T, n_insert, n, 1, 4, 1);      // the inserted values take the block's place
  if ((rc = ensure(ctx, &ctx->greedy, &ctx->cap_greedy, b.doubles))) return rc;
  double* w = ctx->greedy;
  double2* front = (double2*)(w + b.front);
  int *size = (int*)(w + b.size), *flag = (int*)(w + b.flag);
  GPBO_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
  if (n > 0)
    GPBO_HIP(ctx, hipMemcpyAsync(w + b.basev, base_values, (size_t)2 * T * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (n_insert > 0)
    GPBO_HIP(ctx, hipMemcpyAsync(w + b.vals, insert_values, (size_t)2 * T * n_insert * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  qnehvi_front_kernel<<<dim3((unsigned)T), dim3(QNEI_BLOCK), 0, ctx->stream>>>(w + b.basev, w + b.basev + (int64_t)T * n, n, n, ref[0],
                                                                              ref[1], T, front, (double2*)(w + b.front0), size,
                                                                              (int*)(w + b.size0), flag);
  GPBO_HIP(ctx, hipGetLastError());
  if (n_insert > 0) {
    qnehvi_insert_kernel<<<dim3((unsigned)((T + QNEI_BLOCK - 1) / QNEI_BLOCK)), dim3(QNEI_BLOCK), 0, ctx->stream>>>(
        w + b.vals, n_insert, n_insert, T, ref[0], ref[1], front, size, flag);
    GPBO_HIP(ctx, hipGetLastError());
  }
  int over = 0;
  GPBO_HIP(ctx, hipMemcpyAsync(&over, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(front_size_out, size, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(fronts_out, front, (size_t)T * QNEHVI_FRONT * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (over) return qnehvi_overflow(ctx, "debug_qnehvi_fronts", T, over);
  return GPBO_OK;
}
#endif

int launch_qnehvi_greedy(gpbo_ctx* ctx, const Model* const* ms, int64_t M, const double* y_mean, const double* y_std, int G, int S,
                         int F, const double* omega, const double* phase, const double* weights, const double* eps, const double* ref,
                         const double* base_pts, int B, int q, int64_t index_offset, int64_t* pick_idx, double* pick_gain,
                         int* front_size_out, double* fronts_out, double* values_out, double* base_values_out, double* keys_out) {
  int rc;
  const int d = ms[0]->d, DP = ms[0]->DP, T = G * S;
  const QnehviBlock b = qnehvi_block(T, M, B, d, DP, q);
  if ((rc = ensure(ctx, &ctx->greedy, &ctx->cap_greedy, b.doubles))) return rc;
  double* w = ctx->greedy;
  double *vals = w + b.vals, *basev = w + b.basev;
  double2 *front = (double2*)(w + b.front), *front0 = (double2*)(w + b.front0);
  int *size = (int*)(w + b.size), *size0 = (int*)(w + b.size0), *flag = (int*)(w + b.flag);
  uint8_t* mask = (uint8_t*)(w + b.mask);
  GreedyRecord* rec = (GreedyRecord*)(w + b.rec);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  greedy_mark(ctx, ctx->qnehvi_clock, 0);
  GPBO_HIP(ctx, hipMemsetAsync(mask, 0, (size_t)((M + 7) / 8 * 8), ctx->stream));
  GPBO_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
  if (B > 0) GPBO_HIP(ctx, hipMemcpyAsync(w + b.base, base_pts, (size_t)B * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  // the draws, slot by slot (the candidates and the base points scaled by the slot's length scales) and group by group: the
  // group's inputs and path weights into the paths workspace, then its S rows of each buffer
  const GreedyDraws draws = greedy_draws(2, ms, G, S, F, omega, phase, weights, eps);
  for (int j = 0; j < 2; ++j) {
    const Model& m = *ms[j];
    double* base_s = w + b.base_s + (int64_t)j * B * DP;
    if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
    if (B > 0 && (rc = launch_prescale(ctx, w + b.base, B, d, DP, m.ls, base_s, B))) return rc;
    for (int g = 0; g < G; ++g) {
      PathWorkspace ws{};
      if ((rc = greedy_path_weights(ctx, draws, m, j, g, &ws))) return rc;
      const int64_t row = (int64_t)j * T + (int64_t)g * S;
      if ((rc = launch_paths_over(ctx, m, ws, y_mean[j], y_std[j], S, F, ctx->Xcs, M, vals + row * M, M))) return rc;
      if (B > 0 && (rc = launch_paths_over(ctx, m, ws, y_mean[j], y_std[j], S, F, base_s, B, basev + row * b.ldb, b.ldb))) return rc;
    }
  }
  greedy_mark(ctx, ctx->qnehvi_clock, 1);
  const dim3 block(QNEI_BLOCK);
  qnehvi_front_kernel<<<dim3((unsigned)T), block, 0, ctx->stream>>>(basev, basev + (int64_t)T * b.ldb, b.ldb, B, ref[0], ref[1], T, front,
                                                                    front0, size, size0, flag);
  GPBO_HIP(ctx, hipGetLastError());
  greedy_mark(ctx, ctx->qnehvi_clock, 2);
  const int items = qnei_items(M);
  const dim3 grid((unsigned)qnei_score_blocks(M));
  rc = greedy_steps(
      ctx, M, q, keys_out,
      [&] {
        if (items == 2) qnehvi_score_kernel<2><<<grid, block, 0, ctx->stream>>>(vals, M, T, front, size, ref[0], ref[1], mask, ctx->ys);
        else qnehvi_score_kernel<1><<<grid, block, 0, ctx->stream>>>(vals, M, T, front, size, ref[0], ref[1], mask, ctx->ys);
      },
      [&](const SelState* st, const Key* first, int j) {
        qnehvi_update_kernel<<<dim3(1), block, 0, ctx->stream>>>(st, first, vals, M, T, index_offset, j, ref[0], ref[1], front, size,
                                                                 mask, rec, flag);
      });
  if (rc) return rc;
  greedy_mark(ctx, ctx->qnehvi_clock, 3);
  const GreedyRecord* hrec;
  int over = 0;
  const size_t front_bytes = (size_t)T * QNEHVI_FRONT * 2 * sizeof(double);
  if ((rc = greedy_fetch(ctx, rec, q, &hrec))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(&over, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (front_size_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(front_size_out, size0, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipMemcpyAsync(front_size_out + T, size, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (fronts_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(fronts_out, front0, front_bytes, hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipMemcpyAsync(fronts_out + (size_t)T * QNEHVI_FRONT * 2, front, front_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (values_out)
    GPBO_HIP(ctx, hipMemcpyAsync(values_out, vals, (size_t)2 * T * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (base_values_out && B > 0)
    GPBO_HIP(ctx, hipMemcpyAsync(base_values_out, basev, (size_t)2 * T * (size_t)B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (over) return qnehvi_overflow(ctx, "qnehvi_greedy", T, over);
  for (int j = 0; j < q; ++j) { pick_idx[j] = hrec[j].idx; pick_gain[j] = hrec[j].gain; }
  return GPBO_OK;
}

// ---- gpmo_cnhvi_greedy ------------------------------------------------------------------------------------------------------

struct CnhviRecord { double gain; int64_t idx; double feasible; };      // gpmo_cnhvi_greedy's (greedy_fetch checks its room)
static_assert(sizeof(CnhviRecord) == 24, "a record is three doubles of the workspace");

// qnehvi_update_kernel's work over the block whose objective 0 is masked, plus feasible = (the number of draws t whose masked value
// at the pick is > -inf) / T: NaN for a NaN pick.  An infeasible draw's (-inf, y1) fails qnehvi_insert's first test.
__global__ __launch_bounds__(QNEI_BLOCK) void cnhvi_update_kernel(const SelState* __restrict__ st, const Key* __restrict__ first,
                                                                  const double* __restrict__ vals, int64_t M, int T, int64_t offset,
                                                                  int j, double ref0, double ref1, double2* __restrict__ front,
                                                                  int* __restrict__ size, uint8_t* __restrict__ mask,
                                                                  CnhviRecord* __restrict__ rec, int* __restrict__ flag) {
  __shared__ int count;
  if (threadIdx.x == 0) count = 0;
  __syncthreads();
  const GreedyPick p = greedy_pick(st, first, M, offset);
  const int64_t pick = p.local;
  const int t = threadIdx.x;
  if (pick >= 0 && t < T) {
    const double y0 = vals[(int64_t)t * M + pick], y1 = vals[((int64_t)T + t) * M + pick];
    if (y0 > -std::numeric_limits<double>::infinity()) atomicAdd(&count, 1);
    if (qnehvi_insert(front + (int64_t)t * QNEHVI_FRONT, size + t, y0, y1, ref0, ref1)) atomicMax(flag, T - t);
  }
  __syncthreads();
  if (t == 0) {
    rec[j] = CnhviRecord{p.gain, p.idx, (p.nan || pick < 0) ? std::numeric_limits<double>::quiet_NaN() : (double)count / (double)T};
    if (pick >= 0) mask[pick] = 1;
  }
}

int launch_cnhvi_greedy(gpbo_ctx* ctx, int C, const Model* const* ms, int64_t M, const double* y_mean, const double* y_std,
                        const double* lb, const double* ub, int G, int S, int F, const double* omega, const double* phase,
                        const double* weights, const double* eps, const double* ref, const double* base_pts, int B, int q,
                        int64_t index_offset, int64_t* pick_idx, double* pick_gain, double* pick_feasible, int* front_size_out,
                        double* fronts_out, double* values_out, double* viol_out, double* base_values_out, double* keys_out) {
  int rc;
  const int d = ms[0]->d, DP = ms[0]->DP, T = G * S;
  const bool keep_base = base_values_out != nullptr && B > 0;
  const CmoBlock b = cmo_block(T, S, M, B, d, DP, q, values_out != nullptr, keep_base);
  if ((rc = ensure(ctx, &ctx->greedy, &ctx->cap_greedy, b.doubles))) return rc;
  double* w = ctx->greedy;
  double *vals = w + b.vals, *basev = w + b.basev, *viol = w + b.viol, *violb = w + b.violb, *base_s = w + b.base_s;
  double* stage = values_out ? w + b.stage : nullptr;
  double* stageb = keep_base ? w + b.stageb : nullptr;
  double2 *front = (double2*)(w + b.front), *front0 = (double2*)(w + b.front0);
  int *size = (int*)(w + b.size), *size0 = (int*)(w + b.size0), *flag = (int*)(w + b.flag);
  uint8_t* mask = (uint8_t*)(w + b.mask);
  CnhviRecord* rec = (CnhviRecord*)(w + b.rec);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  greedy_mark(ctx, ctx->cnhvi_clock, 0);
  GPBO_HIP(ctx, hipMemsetAsync(mask, 0, (size_t)((M + 7) / 8 * 8), ctx->stream));
  GPBO_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
  if (B > 0) GPBO_HIP(ctx, hipMemcpyAsync(w + b.base, base_pts, (size_t)B * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const GreedyDraws draws = greedy_draws(2 + C, ms, G, S, F, omega, phase, weights, eps);
  // the draws, group by group; per group the constraints in slot order (the violation's sum order), then objective 0 through the
  // mask, then objective 1 as it is: per slot the group's path weights, the candidates and the base points scaled by THAT slot's
  // length scales, one pass over each
  const size_t cand_bytes = (size_t)S * (size_t)M * sizeof(double), base_bytes = (size_t)S * (size_t)B * sizeof(double);
  for (int g = 0; g < G; ++g) {
    const int64_t row = (int64_t)g * S;
    for (int k = 0; k < C + 2; ++k) {
      const int j = k < C ? 2 + k : k - C;      // 2 .. 1 + C, 0, 1
      const Model& m = *ms[j];
      PathWorkspace ws{};
      if ((rc = greedy_path_weights(ctx, draws, m, j, g, &ws))) return rc;
      if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
      if (B > 0 && (rc = launch_prescale(ctx, w + b.base, B, d, DP, m.ls, base_s, B))) return rc;
      double* out = vals + ((int64_t)j * T + row) * M;                 // (objectives only)
      double* outb = basev + ((int64_t)j * T + row) * b.ldb;
      if (j == 1) {
        if ((rc = launch_paths_over(ctx, m, ws, y_mean[j], y_std[j], S, F, ctx->Xcs, M, out, M))) return rc;
        if (values_out)
          GPBO_HIP(ctx, hipMemcpyAsync(values_out + ((int64_t)j * T + row) * M, out, cand_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (B > 0 && (rc = launch_paths_over(ctx, m, ws, y_mean[j], y_std[j], S, F, base_s, B, outb, b.ldb))) return rc;
        if (keep_base)
          GPBO_HIP(ctx, hipMemcpyAsync(base_values_out + ((int64_t)j * T + row) * B, outb, base_bytes, hipMemcpyDeviceToHost, ctx->stream));
        continue;
      }
      const int epilogue = j == 0 ? (int)PATH_MASKED : (j == 2 ? (int)PATH_VIOL_WRITE : (int)PATH_VIOL_ADD);
      const double lo = j ? lb[j - 2] : 0.0, hi = j ? ub[j - 2] : 0.0;
      if ((rc = launch_paths_over_fold(ctx, m, ws, y_mean[j], y_std[j], S, F, ctx->Xcs, M, j ? nullptr : out, M,
                                       PathFold{epilogue, lo, hi, viol, stage})))
        return rc;
      if (values_out)      // stream order: the next pass overwrites the stage after this copy has read it
        GPBO_HIP(ctx, hipMemcpyAsync(values_out + ((int64_t)j * T + row) * M, stage, cand_bytes, hipMemcpyDeviceToHost, ctx->stream));
      if (B > 0) {
        if ((rc = launch_paths_over_fold(ctx, m, ws, y_mean[j], y_std[j], S, F, base_s, B, j ? nullptr : outb, b.ldb,
                                         PathFold{epilogue, lo, hi, violb, stageb})))
          return rc;
        if (keep_base)
          GPBO_HIP(ctx, hipMemcpyAsync(base_values_out + ((int64_t)j * T + row) * B, stageb, base_bytes, hipMemcpyDeviceToHost, ctx->stream));
      }
      if (j == 0 && viol_out) GPBO_HIP(ctx, hipMemcpyAsync(viol_out + row * M, viol, cand_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  greedy_mark(ctx, ctx->cnhvi_clock, 1);
  const dim3 block(QNEI_BLOCK);
  qnehvi_front_kernel<<<dim3((unsigned)T), block, 0, ctx->stream>>>(basev, basev + (int64_t)T * b.ldb, b.ldb, B, ref[0], ref[1], T, front,
                                                                    front0, size, size0, flag);
  GPBO_HIP(ctx, hipGetLastError());
  greedy_mark(ctx, ctx->cnhvi_clock, 2);
  const int items = qnei_items(M);
  const dim3 grid((unsigned)qnei_score_blocks(M));
  rc = greedy_steps(
      ctx, M, q, keys_out,
      [&] {
        if (items == 2) qnehvi_score_kernel<2><<<grid, block, 0, ctx->stream>>>(vals, M, T, front, size, ref[0], ref[1], mask, ctx->ys);
        else qnehvi_score_kernel<1><<<grid, block, 0, ctx->stream>>>(vals, M, T, front, size, ref[0], ref[1], mask, ctx->ys);
      },
      [&](const SelState* st, const Key* first, int j) {
        cnhvi_update_kernel<<<dim3(1), block, 0, ctx->stream>>>(st, first, vals, M, T, index_offset, j, ref[0], ref[1], front, size,
                                                                mask, rec, flag);
      });
  if (rc) return rc;
  greedy_mark(ctx, ctx->cnhvi_clock, 3);
  const CnhviRecord* hrec;
  int over = 0;
  const size_t front_bytes = (size_t)T * QNEHVI_FRONT * 2 * sizeof(double);
  if ((rc = greedy_fetch(ctx, rec, q, &hrec))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(&over, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (front_size_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(front_size_out, size0, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipMemcpyAsync(front_size_out + T, size, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (fronts_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(fronts_out, front0, front_bytes, hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipMemcpyAsync(fronts_out + (size_t)T * QNEHVI_FRONT * 2, front, front_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (over) return qnehvi_overflow(ctx, "cnhvi_greedy", T, over);
  for (int j = 0; j < q; ++j) { pick_idx[j] = hrec[j].idx; pick_gain[j] = hrec[j].gain; pick_feasible[j] = hrec[j].feasible; }
  return GPBO_OK;
}

}  // namespace gpbo
