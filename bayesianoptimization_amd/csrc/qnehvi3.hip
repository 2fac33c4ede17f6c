// gpmo3_nhvi_greedy (gfx950): a batch of q candidates by greedy noisy expected hypervolume improvement over T joint posterior draws
// of m = 3 objectives (include/gpmo3.h has the rule and the conventions; qnehvi3_plan.h the workspace and the packing of the score
// kernel's LDS stages).  What gpbo_qnhvi_greedy (qnehvi.hip) does for two objectives, with a box decomposition per draw in place of
// the staircase's strips.
//
// The draws' values are made by the kernels of gpbo_sample_paths (launch_path_weights, launch_paths_over), slot by slot and group by
// group, into a resident (3, T, M) block and a small [3][T][B] buffer at the base points; the step loop, the pick rule and the draws'
// input layout are greedy.h's.  New here:
//   qnehvi3_sweep          the decomposition, one wave: the front's points in stored order (objective 2 descending) against a 2-D
//                          staircase S in LDS.  Per point: its place p and the run [p, r) it covers by two ballots, the r - p + 1
//                          rectangles it covers FIRST — lane = rectangle, compacted by a ballot's prefix, in emission order — at the
//                          point's height, then S[p, r) replaced by the point (lane = entry, through registers).  Then the ground.
//                          At most 2 n + 1 cells of five doubles
//   qnehvi3_front_kernel   a workgroup per draw: the front from the draw's B value triples by repeated block-wide lexicographic
//                          arg-max over the LIVE triples (a 64-bit mask per thread: 64 x 256 = GPBO_MAX_QNEHVI_BASE); after a point is
//                          accepted every thread drops the triples it covers in objectives (0, 1) — they are not above it in
//                          objective 2, so they are dominated or equal.  O(B n / 256) per thread, no sort, no n^2 test; the front
//                          comes out in sweep order and wave 0 sweeps it
//   qnehvi3_score_kernel   the hot loop, once per greedy step: thread = one or two candidates (qnei_items), walking the T rows of the
//                          three blocks with four draws' rows in flight; the cells staged in LDS, a stage packed by the draws' actual
//                          cell counts (qnehvi3_stage_draws), and read back as wave-wide broadcasts of 16 + 16 + 8 bytes
//   qnehvi3_update_kernel  a wave per draw behind the step's selection: the pick (greedy_pick), {gain, index} and the mask by draw 0's
//                          wave; every wave inserts its draw's triple at the pick (qnehvi3_absorb: lane = point) and re-sweeps where
//                          the front changed
// No multiply-add in any of them (the file is compiled with -ffp-contract=off as well): tests replay the keys bit for bit.
#include "greedy.h"
#include "qnehvi3_plan.h"

#include <cmath>
#include <limits>
#include <string>

namespace gpbo {

static_assert(GPBO_MAX_QNEHVI_BASE <= 64 * QNEI_BLOCK, "qnehvi3_front_kernel keeps a thread's live triples in one 64-bit mask");
static_assert(QNEHVI3_FRONT <= 2 * QNEHVI3_WAVE, "a lane holds two points of a front / two entries of the staircase");

// the lanes of one wave agree on LDS: what was written before is read after
__device__ __forceinline__ void qnehvi3_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int qnehvi3_votes(bool p) { return __popcll(__ballot(p)); }

__device__ __forceinline__ void qnehvi3_put(double* __restrict__ o, double x_lo, double x_hi, double y_lo, double y_hi, double h) {
  o[0] = x_lo; o[1] = x_hi; o[2] = y_lo; o[3] = y_hi; o[4] = h;
}

// The cells of the front (fx, fy, fz)[0 .. n) (LDS, stored order) into out[QNEHVI3_CELLS][5] (and out0, where given), by ONE WAVE
// (lane = its lane); sx, sy: LDS room for the staircase, QNEHVI3_FRONT entries each.  Returns the number of cells, cut at
// QNEHVI3_CELLS (the rule never emits more; nothing is written past the arrays whatever the input).
__device__ int qnehvi3_sweep(const double* fx, const double* fy, const double* fz, int n, double ref0, double ref1, double ref2,
                             double* sx, double* sy, double* __restrict__ out, double* __restrict__ out0, int lane) {
  const double inf = std::numeric_limits<double>::infinity();
  const uint64_t below = (1ull << lane) - 1;
  int m = 0, nc = 0;
  auto emit = [&](bool store, double x_lo, double x_hi, double y_lo, double y_hi, double h) {
    const uint64_t votes = __ballot(store);
    const int at = nc + __popcll(votes & below);
    if (store && at < QNEHVI3_CELLS) {
      qnehvi3_put(out + (int64_t)at * QNEHVI3_CELL, x_lo, x_hi, y_lo, y_hi, h);
      if (out0) qnehvi3_put(out0 + (int64_t)at * QNEHVI3_CELL, x_lo, x_hi, y_lo, y_hi, h);
    }
    nc += __popcll(votes);
  };
  qnehvi3_wave_sync();      // the caller's writes of the front
  for (int i = 0; i < n; ++i) {
    const double a = fx[i], b = fy[i], c = fz[i];
    int p = 0, run = 0;      // S is sorted: the entries right of a are [0, p), those not right of a and not above b are [p, p + run)
    for (int k0 = 0; k0 < m; k0 += QNEHVI3_WAVE) {
      const int k = k0 + lane;
      const bool in = k < m;
      const bool right = in && sx[k] > a;
      p += qnehvi3_votes(right);
      run += qnehvi3_votes(in && !right && sy[k] <= b);
    }
    const int r = p + run;
    for (int k0 = p; k0 <= r; k0 += QNEHVI3_WAVE) {
      const int k = k0 + lane;
      const bool in = k <= r;
      const double x_hi = !in ? 0.0 : (k == p ? a : sx[k - 1]);
      const double x_lo = !in ? 0.0 : (k < m ? sx[k] : ref0);
      const double y_lo = !in ? 0.0 : (k > 0 ? sy[k - 1] : ref1);
      emit(in && x_hi != x_lo, x_lo, x_hi, y_lo, b, c);
    }
    // S[p, r) becomes (a, b): the tail [r, m) moves by 1 - run, through registers
    const int shift = 1 - run;
    double tx[2] = {0.0, 0.0}, ty[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = r + lane + h * QNEHVI3_WAVE;
      if (k < m) { tx[h] = sx[k]; ty[h] = sy[k]; }
    }
    qnehvi3_wave_sync();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = r + lane + h * QNEHVI3_WAVE;
      if (shift != 0 && k < m && k + shift < QNEHVI3_FRONT) { sx[k + shift] = tx[h]; sy[k + shift] = ty[h]; }
    }
    if (lane == 0 && p < QNEHVI3_FRONT) { sx[p] = a; sy[p] = b; }
    m += shift;
    if (m > QNEHVI3_FRONT) m = QNEHVI3_FRONT;
    qnehvi3_wave_sync();
  }
  for (int k0 = 0; k0 <= m; k0 += QNEHVI3_WAVE) {      // the ground: the strips of the final staircase
    const int k = k0 + lane;
    const bool in = k <= m;
    const double x_hi = (!in || k == 0) ? inf : sx[k - 1];
    const double x_lo = !in ? 0.0 : (k < m ? sx[k] : ref0);
    const double y_lo = !in ? 0.0 : (k > 0 ? sy[k - 1] : ref1);
    emit(in, x_lo, x_hi, y_lo, inf, ref2);
  }
  return nc < QNEHVI3_CELLS ? nc : QNEHVI3_CELLS;
}

// (x, y, z) < (ox, oy, oz) in the stored order's arg-max: objective 2, then objective 0, then objective 1
__device__ __forceinline__ bool qnehvi3_less(double x, double y, double z, double ox, double oy, double oz) {
  return oz > z || (oz == z && (ox > x || (ox == x && oy > y)));
}

// The front of draw t = blockIdx.x from the triples (v0, v1, v2)[t ld + i], i < n <= GPBO_MAX_QNEHVI_BASE, and its cells; every
// output twice: the live copy and the one the call hands back as "before the first pick".  A front of more than QNEHVI3_FRONT
// points raises the flag (T - t: the lowest draw stays) and is cut there.
__global__ __launch_bounds__(QNEI_BLOCK) void qnehvi3_front_kernel(const double* __restrict__ v0, const double* __restrict__ v1,
                                                                   const double* __restrict__ v2, int64_t ld, int n, double ref0,
                                                                   double ref1, double ref2, int T, double* __restrict__ front,
                                                                   double* __restrict__ front0, double* __restrict__ cells,
                                                                   double* __restrict__ cells0, int* __restrict__ size,
                                                                   int* __restrict__ size0, int* __restrict__ ncell,
                                                                   int* __restrict__ ncell0, int* __restrict__ flag) {
  __shared__ double fx[QNEHVI3_FRONT], fy[QNEHVI3_FRONT], fz[QNEHVI3_FRONT], sx[QNEHVI3_FRONT], sy[QNEHVI3_FRONT];
  __shared__ double wx[QNEI_BLOCK / 64], wy[QNEI_BLOCK / 64], wz[QNEI_BLOCK / 64];
  __shared__ double best[3];
  const int t = blockIdx.x, tid = threadIdx.x;
  const double* r0 = v0 + (int64_t)t * ld;
  const double* r1 = v1 + (int64_t)t * ld;
  const double* r2 = v2 + (int64_t)t * ld;
  const double none = -std::numeric_limits<double>::infinity();      // ref2 is finite: every live triple is above it
  uint64_t live = 0;      // bit k: triple tid + k QNEI_BLOCK is above ref, holds no NaN and is not covered yet
  for (int k = 0; k < 64; ++k) {
    const int i = tid + k * QNEI_BLOCK;
    if (i < n && r0[i] > ref0 && r1[i] > ref1 && r2[i] > ref2) live |= 1ull << k;      // a NaN fails a comparison
  }
  double pa = 0.0, pb = 0.0;
  int count = 0;
  for (int round = 0; round <= QNEHVI3_FRONT; ++round) {
    double x = none, y = none, z = none;
    for (uint64_t left = live; left; left &= left - 1) {
      const int k = __ffsll((unsigned long long)left) - 1;
      const int i = tid + k * QNEI_BLOCK;
      const double ox = r0[i], oy = r1[i];
      if (round > 0 && ox <= pa && oy <= pb) { live &= ~(1ull << k); continue; }      // covered by the last accepted point
      const double oz = r2[i];
      if (qnehvi3_less(x, y, z, ox, oy, oz)) { x = ox; y = oy; z = oz; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ox = __shfl_xor(x, o), oy = __shfl_xor(y, o), oz = __shfl_xor(z, o);
      if (qnehvi3_less(x, y, z, ox, oy, oz)) { x = ox; y = oy; z = oz; }
    }
    if ((tid & 63) == 0) { wx[tid >> 6] = x; wy[tid >> 6] = y; wz[tid >> 6] = z; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < QNEI_BLOCK / 64; ++w)
        if (qnehvi3_less(x, y, z, wx[w], wy[w], wz[w])) { x = wx[w]; y = wy[w]; z = wz[w]; }
      best[0] = x; best[1] = y; best[2] = z;
    }
    __syncthreads();
    x = best[0]; y = best[1]; z = best[2];
    if (z == none) break;
    if (count == QNEHVI3_FRONT) {
      if (tid == 0) atomicMax(flag, T - t);
      break;
    }
    if (tid == 0) {
      fx[count] = x; fy[count] = y; fz[count] = z;
      double* f = front + ((int64_t)t * QNEHVI3_FRONT + count) * 3;
      double* f0 = front0 + ((int64_t)t * QNEHVI3_FRONT + count) * 3;
      f[0] = x; f[1] = y; f[2] = z;
      f0[0] = x; f0[1] = y; f0[2] = z;
    }
    ++count;
    pa = x; pb = y;
  }
  __syncthreads();      // the front stands in LDS
  if (tid >= QNEHVI3_WAVE) return;
  const int64_t at = (int64_t)t * QNEHVI3_CELLS * QNEHVI3_CELL;
  const int nc = qnehvi3_sweep(fx, fy, fz, count, ref0, ref1, ref2, sx, sy, cells + at, cells0 + at, tid);
  if (tid == 0) { size[t] = count; size0[t] = count; ncell[t] = nc; ncell0[t] = nc; }
}

// The update rule of one draw, by ONE WAVE: its front gf[0 .. *gsize) (global, stored order) absorbs y.  Unchanged if y has a NaN, is
// not strictly above ref in all three, or is dominated by or equal to a point; else the points y dominates leave, y enters in its
// sorted place, and the cells are rebuilt.  true: the front would outgrow QNEHVI3_FRONT (it is left as it is).
__device__ bool qnehvi3_absorb(double* __restrict__ gf, int* __restrict__ gsize, double* __restrict__ gcells, int* __restrict__ gncell,
                               double y0, double y1, double y2, double ref0, double ref1, double ref2, double* fx, double* fy,
                               double* fz, double* sx, double* sy, int lane) {
  if (!(y0 > ref0 && y1 > ref1 && y2 > ref2)) return false;
  const uint64_t below = (1ull << lane) - 1;
  int n = *gsize;
  if (n > QNEHVI3_FRONT) n = QNEHVI3_FRONT;
  double px[2], py[2], pz[2];
  bool keep[2];
  int to[2];
  int kept = 0, ahead = 0;      // points that stay | those of them that precede y in the stored order (a prefix: the front is sorted)
  bool covered = false;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + h * QNEHVI3_WAVE;
    const bool has = k < n;
    px[h] = has ? gf[k * 3] : 0.0; py[h] = has ? gf[k * 3 + 1] : 0.0; pz[h] = has ? gf[k * 3 + 2] : 0.0;
    covered |= __ballot(has && px[h] >= y0 && py[h] >= y1 && pz[h] >= y2) != 0;
    keep[h] = has && !(px[h] <= y0 && py[h] <= y1 && pz[h] <= y2);
    const uint64_t votes = __ballot(keep[h]);
    to[h] = kept + __popcll(votes & below);
    kept += __popcll(votes);
    ahead += qnehvi3_votes(keep[h] && qnehvi3_less(y0, y1, y2, px[h], py[h], pz[h]));
  }
  if (covered) return false;
  if (kept + 1 > QNEHVI3_FRONT) return true;
  qnehvi3_wave_sync();      // every lane has read its points
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (!keep[h]) continue;
    const int k = to[h] < ahead ? to[h] : to[h] + 1;
    fx[k] = px[h]; fy[k] = py[h]; fz[k] = pz[h];
    gf[k * 3] = px[h]; gf[k * 3 + 1] = py[h]; gf[k * 3 + 2] = pz[h];
  }
  if (lane == 0) {
    fx[ahead] = y0; fy[ahead] = y1; fz[ahead] = y2;
    gf[ahead * 3] = y0; gf[ahead * 3 + 1] = y1; gf[ahead * 3 + 2] = y2;
    *gsize = kept + 1;
  }
  const int nc = qnehvi3_sweep(fx, fy, fz, kept + 1, ref0, ref1, ref2, sx, sy, gcells, nullptr, lane);
  if (lane == 0) *gncell = nc;
  return false;
}

constexpr int QNEHVI3_AHEAD = 4;      // draws whose rows a thread has in flight before it walks their cells

// key_j over the candidates: ITEMS (qnei_plan.h: qnei_items) neighbouring candidates per thread, read as one load per row and objective
template <int ITEMS>
__global__ __launch_bounds__(QNEI_BLOCK) void qnehvi3_score_kernel(const double* __restrict__ vals, int64_t M, int T,
                                                                   const double* __restrict__ cells, const int* __restrict__ ncell,
                                                                   const uint8_t* __restrict__ mask, double* __restrict__ ys) {
  __shared__ double2 cx[QNEHVI3_STAGE_CELLS], cy[QNEHVI3_STAGE_CELLS];
  __shared__ double ch[QNEHVI3_STAGE_CELLS];
  __shared__ int first[QNEHVI3_STAGE_DRAWS + 1];
  static_assert(sizeof(cx) + sizeof(cy) + sizeof(ch) + sizeof(first) == QNEHVI3_LDS_BYTES, "qnehvi3_plan.h states the stage's size");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t i = qnei_first_candidate(blockIdx.x, tid, ITEMS);
  const bool live = i < M;      // (with ITEMS == 2 M is even: i + 1 < M too, and every row's pair sits on a 16-byte boundary)
  const double* col = vals + (live ? i : 0);
  const int64_t plane = (int64_t)T * M;
  const double inf = std::numeric_limits<double>::infinity();
  double s[ITEMS];
#pragma unroll
  for (int c = 0; c < ITEMS; ++c) s[c] = 0.0;
  for (int t0 = 0; t0 < T;) {
    int total;
    const int C = qnehvi3_stage_draws(ncell, t0, T, &total);      // uniform: the counts are the same for every thread
    __syncthreads();      // the stage before this one has been read
    int at = 0;
    for (int tl = 0; tl < C; ++tl) {      // wave w stages draws w, w + 4, ...: lane = cell
      const int n = qnehvi3_count(ncell[t0 + tl]);
      if (tid == 0) first[tl] = at;
      if ((tl & (QNEI_BLOCK / 64 - 1)) == wave) {
        const double* g = cells + (int64_t)(t0 + tl) * QNEHVI3_CELLS * QNEHVI3_CELL;
        for (int k = lane; k < n; k += 64) {
          const double* e = g + k * QNEHVI3_CELL;
          cx[at + k] = make_double2(e[0], e[1]);
          cy[at + k] = make_double2(e[2], e[3]);
          ch[at + k] = e[4];
        }
      }
      at += n;
    }
    if (tid == 0) first[C] = at;
    __syncthreads();
    if (live) {
      for (int tl = 0; tl < C; tl += QNEHVI3_AHEAD) {
        double f[QNEHVI3_AHEAD][3][ITEMS];
#pragma unroll
        for (int u = 0; u < QNEHVI3_AHEAD; ++u) {
          const int64_t row = (int64_t)(t0 + (tl + u < C ? tl + u : C - 1)) * M;      // (past the stage: its last row again, unused)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            if (ITEMS == 2) {
              const double2 v = *reinterpret_cast<const double2*>(col + j * plane + row);
              f[u][j][0] = v.x; f[u][j][ITEMS - 1] = v.y;
            } else {
              f[u][j][0] = col[j * plane + row];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < QNEHVI3_AHEAD; ++u) {
          if (tl + u >= C) break;
          const int k1 = first[tl + u + 1];
          double hvi[ITEMS];
#pragma unroll
          for (int c = 0; c < ITEMS; ++c) hvi[c] = 0.0;
          for (int k = first[tl + u]; k < k1; ++k) {
            const double2 X = cx[k], Y = cy[k];
            const double h = ch[k];
#pragma unroll
            for (int c = 0; c < ITEMS; ++c) {
              const double f0 = f[u][0][c], f1 = f[u][1][c];
              const double w = (f0 < X.y ? f0 : X.y) - X.x, v = (f1 < Y.y ? f1 : Y.y) - Y.x, z = f[u][2][c] - h;
              const double area = (w > 0.0 ? w : 0.0) * (v > 0.0 ? v : 0.0);
              hvi[c] += area * (z > 0.0 ? z : 0.0);
            }
          }
#pragma unroll
          for (int c = 0; c < ITEMS; ++c) {
            const double f0 = f[u][0][c], f1 = f[u][1][c], f2 = f[u][2][c];
            s[c] += (f0 != f0 || f1 != f1 || f2 != f2) ? std::numeric_limits<double>::quiet_NaN() : hvi[c];
          }
        }
      }
    }
    t0 += C;
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

// Behind step j's selection, a wave per draw t = blockIdx.x: the pick (greedy_pick), its record and the mask (draw 0's wave), the
// draw's front and cells (qnehvi3_absorb).
__global__ __launch_bounds__(QNEHVI3_WAVE) void qnehvi3_update_kernel(const SelState* __restrict__ st, const Key* __restrict__ sel,
                                                                      const double* __restrict__ vals, int64_t M, int T,
                                                                      int64_t offset, int j, double ref0, double ref1, double ref2,
                                                                      double* __restrict__ front, int* __restrict__ size,
                                                                      double* __restrict__ cells, int* __restrict__ ncell,
                                                                      uint8_t* __restrict__ mask, GreedyRecord* __restrict__ rec,
                                                                      int* __restrict__ flag) {
  __shared__ double fx[QNEHVI3_FRONT], fy[QNEHVI3_FRONT], fz[QNEHVI3_FRONT], sx[QNEHVI3_FRONT], sy[QNEHVI3_FRONT];
  const GreedyPick p = greedy_pick(st, sel, M, offset);
  const int64_t pick = p.local;
  const int t = blockIdx.x, lane = threadIdx.x;
  if (t == 0 && lane == 0) {
    rec[j] = GreedyRecord{p.gain, p.idx};
    if (pick >= 0) mask[pick] = 1;
  }
  if (pick < 0) return;
  const int64_t plane = (int64_t)T * M;
  const double* v = vals + (int64_t)t * M + pick;
  const bool over = qnehvi3_absorb(front + (int64_t)t * QNEHVI3_FRONT * 3, size + t, cells + (int64_t)t * QNEHVI3_CELLS * QNEHVI3_CELL,
                                   ncell + t, v[0], v[plane], v[2 * plane], ref0, ref1, ref2, fx, fy, fz, sx, sy, lane);
  if (over && lane == 0) atomicMax(flag, T - t);
}

// the refusal behind the call's one synchronisation: flag = T - t for the lowest draw t whose front outgrew its array
static int qnehvi3_overflow(gpbo_ctx* ctx, const char* who, int T, int flag) {
  GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, std::string(who) + ": the front of draw " + std::to_string(T - flag) + " outgrew " +
                                           std::to_string(QNEHVI3_FRONT) + " points (GPBO_MAX_QNEHVI_FRONT); a front is never thinned");
}

// the fronts, their cells and both counts on their way home (enqueued): n_blocks = 1: the live state; 2: before the first pick | live
static int qnehvi3_fetch(gpbo_ctx* ctx, const Qnehvi3Block& b, int T, int n_blocks, int* front_size_out, double* fronts_out,
                         int* cell_count_out, double* cells_out) {
  double* w = ctx->greedy;
  const size_t nf = (size_t)T * QNEHVI3_FRONT * 3, ncl = (size_t)T * QNEHVI3_CELLS * QNEHVI3_CELL;
  for (int k = 0; k < n_blocks; ++k) {
    const bool before = n_blocks == 2 && k == 0;
    if (front_size_out)
      GPBO_HIP(ctx, hipMemcpyAsync(front_size_out + (size_t)k * T, w + (before ? b.size0 : b.size), (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (cell_count_out)
      GPBO_HIP(ctx, hipMemcpyAsync(cell_count_out + (size_t)k * T, w + (before ? b.ncell0 : b.ncell), (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (fronts_out)
      GPBO_HIP(ctx, hipMemcpyAsync(fronts_out + k * nf, w + (before ? b.front0 : b.front), nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (cells_out)
      GPBO_HIP(ctx, hipMemcpyAsync(cells_out + k * ncl, w + (before ? b.cells0 : b.cells), ncl * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  return GPBO_OK;
}

static int qnehvi3_build(gpbo_ctx* ctx, const Qnehvi3Block& b, int T, int B, const double* ref) {
  double* w = ctx->greedy;
  const double* basev = w + b.basev;
  qnehvi3_front_kernel<<<dim3((unsigned)T), dim3(QNEI_BLOCK), 0, ctx->stream>>>(
      basev, basev + (int64_t)T * b.ldb, basev + 2 * (int64_t)T * b.ldb, b.ldb, B, ref[0], ref[1], ref[2], T, w + b.front, w + b.front0,
      w + b.cells, w + b.cells0, (int*)(w + b.size), (int*)(w + b.size0), (int*)(w + b.ncell), (int*)(w + b.ncell0), (int*)(w + b.flag));
  GPBO_HIP(ctx, hipGetLastError());
  return GPBO_OK;
}

#ifdef GPBO_DEBUG
// the update rule on given values: the wave of draw t = blockIdx.x absorbs (ins[(j T + t) ld + i])_j, i = 0 .. n_insert - 1 in order
__global__ __launch_bounds__(QNEHVI3_WAVE) void qnehvi3_insert_kernel(const double* __restrict__ ins, int64_t ld, int n_insert, int T,
                                                                      double ref0, double ref1, double ref2, double* __restrict__ front,
                                                                      int* __restrict__ size, double* __restrict__ cells,
                                                                      int* __restrict__ ncell, int* __restrict__ flag) {
  __shared__ double fx[QNEHVI3_FRONT], fy[QNEHVI3_FRONT], fz[QNEHVI3_FRONT], sx[QNEHVI3_FRONT], sy[QNEHVI3_FRONT];
  const int t = blockIdx.x, lane = threadIdx.x;
  const int64_t plane = (int64_t)T * ld;
  for (int i = 0; i < n_insert; ++i) {
    const double* v = ins + (int64_t)t * ld + i;
    if (qnehvi3_absorb(front + (int64_t)t * QNEHVI3_FRONT * 3, size + t, cells + (int64_t)t * QNEHVI3_CELLS * QNEHVI3_CELL, ncell + t,
                       v[0], v[plane], v[2 * plane], ref0, ref1, ref2, fx, fy, fz, sx, sy, lane) && lane == 0)
      atomicMax(flag, T - t);
    __syncthreads();      // (one wave: the next insertion reads what this one wrote)
  }
}

int debug_qnehvi3_cells(gpbo_ctx* ctx, int T, int n, const double* base_values, const double* ref, int n_insert,
                        const double* insert_values, int* front_size_out, double* fronts_out, int* cell_count_out, double* cells_out) {
  int rc;
  const Qnehvi3Block b = qnehvi3_block(T, n_insert, n, 1, 4, 1);      // the inserted values take the block's place
  if ((rc = ensure(ctx, &ctx->greedy, &ctx->cap_greedy, b.doubles))) return rc;
  double* w = ctx->greedy;
  int* flag = (int*)(w + b.flag);
  GPBO_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
  if (n > 0)
    GPBO_HIP(ctx, hipMemcpyAsync(w + b.basev, base_values, (size_t)3 * T * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (n_insert > 0)
    GPBO_HIP(ctx, hipMemcpyAsync(w + b.vals, insert_values, (size_t)3 * T * n_insert * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = qnehvi3_build(ctx, b, T, n, ref))) return rc;
  if (n_insert > 0) {
    qnehvi3_insert_kernel<<<dim3((unsigned)T), dim3(QNEHVI3_WAVE), 0, ctx->stream>>>(
        w + b.vals, n_insert, n_insert, T, ref[0], ref[1], ref[2], w + b.front, (int*)(w + b.size), w + b.cells, (int*)(w + b.ncell), flag);
    GPBO_HIP(ctx, hipGetLastError());
  }
  int over = 0;
  GPBO_HIP(ctx, hipMemcpyAsync(&over, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = qnehvi3_fetch(ctx, b, T, 1, front_size_out, fronts_out, cell_count_out, cells_out))) return rc;
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (over) return qnehvi3_overflow(ctx, "debug_cells", T, over);
  return GPBO_OK;
}
#endif

int launch_qnehvi3_greedy(gpbo_ctx* ctx, const Model* const* ms, int64_t M, const double* y_mean, const double* y_std, int G, int S,
                          int F, const double* omega, const double* phase, const double* weights, const double* eps, const double* ref,
                          const double* base_pts, int B, int q, int64_t index_offset, int64_t* pick_idx, double* pick_gain,
                          int* front_size_out, double* fronts_out, int* cell_count_out, double* cells_out, double* values_out,
                          double* base_values_out, double* keys_out) {
  int rc;
  const int d = ms[0]->d, DP = ms[0]->DP, T = G * S;
  const Qnehvi3Block b = qnehvi3_block(T, M, B, d, DP, q);
  if ((rc = ensure(ctx, &ctx->greedy, &ctx->cap_greedy, b.doubles))) return rc;
  double* w = ctx->greedy;
  double *vals = w + b.vals, *basev = w + b.basev;
  int* flag = (int*)(w + b.flag);
  uint8_t* mask = (uint8_t*)(w + b.mask);
  GreedyRecord* rec = (GreedyRecord*)(w + b.rec);
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  greedy_mark(ctx, ctx->qnehvi3_clock, 0);
  GPBO_HIP(ctx, hipMemsetAsync(mask, 0, (size_t)((M + 7) / 8 * 8), ctx->stream));
  GPBO_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
  if (B > 0) GPBO_HIP(ctx, hipMemcpyAsync(w + b.base, base_pts, (size_t)B * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  // the draws, slot by slot (the candidates and the base points scaled by the slot's length scales) and group by group: the
  // group's inputs and path weights into the paths workspace, then its S rows of each buffer
  const GreedyDraws draws = greedy_draws(3, ms, G, S, F, omega, phase, weights, eps);
  for (int j = 0; j < 3; ++j) {
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
  greedy_mark(ctx, ctx->qnehvi3_clock, 1);
  if ((rc = qnehvi3_build(ctx, b, T, B, ref))) return rc;
  greedy_mark(ctx, ctx->qnehvi3_clock, 2);
  const int items = qnei_items(M);
  const dim3 grid((unsigned)qnei_score_blocks(M)), block(QNEI_BLOCK);
  double* cells = w + b.cells;
  int* ncell = (int*)(w + b.ncell);
  rc = greedy_steps(
      ctx, M, q, keys_out,
      [&] {
        if (items == 2) qnehvi3_score_kernel<2><<<grid, block, 0, ctx->stream>>>(vals, M, T, cells, ncell, mask, ctx->ys);
        else qnehvi3_score_kernel<1><<<grid, block, 0, ctx->stream>>>(vals, M, T, cells, ncell, mask, ctx->ys);
      },
      [&](const SelState* st, const Key* first, int j) {
        qnehvi3_update_kernel<<<dim3((unsigned)T), dim3(QNEHVI3_WAVE), 0, ctx->stream>>>(
            st, first, vals, M, T, index_offset, j, ref[0], ref[1], ref[2], w + b.front, (int*)(w + b.size), cells, ncell, mask, rec, flag);
      });
  if (rc) return rc;
  greedy_mark(ctx, ctx->qnehvi3_clock, 3);
  const GreedyRecord* hrec;
  int over = 0;
  if ((rc = greedy_fetch(ctx, rec, q, &hrec))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(&over, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = qnehvi3_fetch(ctx, b, T, 2, front_size_out, fronts_out, cell_count_out, cells_out))) return rc;
  if (values_out)
    GPBO_HIP(ctx, hipMemcpyAsync(values_out, vals, (size_t)3 * T * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (base_values_out && B > 0)
    GPBO_HIP(ctx, hipMemcpyAsync(base_values_out, basev, (size_t)3 * T * (size_t)B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (over) return qnehvi3_overflow(ctx, "nhvi3_greedy", T, over);
  for (int j = 0; j < q; ++j) { pick_idx[j] = hrec[j].idx; pick_gain[j] = hrec[j].gain; }
  return GPBO_OK;
}

}  // namespace gpbo
