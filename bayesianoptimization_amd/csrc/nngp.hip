// Nearest-neighbour GP scoring of the resident candidates (gfx950): gpnn_acq_argbest's values.  include/gpnn.h has the formulas and
// the conventions; nngp_plan.h the split of the work, the LDS budgets and the workspace.  At fixed hyper-parameters a candidate's
// posterior is the exact GP's conditioned on its k nearest observations: O(N d) for the search, O(k^3) for the solve, no N x N matrix.
// Compiled with -ffp-contract=off (the fmas below are written out).
//
// Four stages:
//   upload   the rows, the targets and the length scales go to the workspace; prescale_kernel (fit_kernels.hip) divides the rows
//            and the resident candidates by the length scales into zero-padded [.][DP] images.
//   search   nn_search_kernel, the hot path: M N distance evaluations of DP fmas each.  Lane = candidate, its scaled coordinates
//            in registers for the whole kernel.  Every wave owns its own 64 candidates; the waves of a workgroup share only the
//            staged chunk of NN_CHUNK rows, which goes through LDS and comes back as broadcasts (the same address in every lane),
//            two rows side by side, so a pair costs DP fmas and no global traffic.  A candidate's current k-list of (d2, index)
//            lives in LDS as [slot][lane]; its worst entry (d2, slot) sits in registers.  The first k rows fill the list.  From
//            then on the rows are walked in ascending index order, so a row enters only if its d2 is STRICTLY below the worst —
//            a tie goes to the lower index, which is already in — and an insert overwrites the worst slot and rescans the k
//            slots for the new worst, the highest index among equal d2 (nn_rescan).  After the first chunks inserts are rare: the i-th row
//            of a random order enters with probability k / i, about k ln(N / k) inserts per candidate against N evaluations.
//            Behind the last chunk a selection sort of the k slots by (d2, index), in LDS, fixes the order for the solve and for
//            nbr_out, and the indices go to the workspace as int32 (-1 for a candidate with a NaN coordinate).
//   solve    nn_solve_kernel.  One wave owns 64 / k candidates, lane = (candidate, row): k = 64 keeps every lane on one
//            candidate, k = 32 / 16 pack 2 / 4 per wave.  A lane gathers its neighbour's scaled row into registers.  The rows
//            take turns through a double-buffered LDS line: in turn j every lane reads row j as a broadcast and writes
//            A[row][j] = c k(d2(X_row, X_j)) for row > j, the forced diagonal for row = j, into the lower triangle in LDS at
//            pitch k + 1.  The factorisation is right-looking, column by column: the pivot is one broadcast read, lane i scales
//            its entry and updates its own row from the column, which the lanes read as broadcasts; the two right-hand sides y_nn
//            and k* ride in registers through the same sweep, lane j's value going round by a lane shuffle.  |v|^2 and v . u
//            are reduced by a fixed butterfly; lane 0 of the candidate writes mu, sd and the acquisition value.  Waves never
//            wait for each other: the sweep's barriers are wave-local.
//   select   the existing arg-best / top-k over ctx->ys (acq_kernels.hip), from the entry point.
// A candidate's bits depend neither on M nor on the other candidates: lists, triangles and sums are per candidate, in a fixed order.
#include "gpbo_internal.h"
#include "acq_formulas.h"
#include "nngp_plan.h"

#include <cmath>

namespace gpbo {

__device__ __forceinline__ void nn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// scaled coordinates of row `r` of a [.][DP] image into registers
template <int DP>
__device__ __forceinline__ void nn_load_row(const double* P, const int64_t r, double (&x)[DP]) {
  const double* p = P + r * DP;
#pragma unroll
  for (int t = 0; t < DP; t += 2) {
    const double2 v = *reinterpret_cast<const double2*>(p + t);
    x[t] = v.x;
    x[t + 1] = v.y;
  }
}

// The list's worst entry under (d2, index): the highest index among the largest d2.  The k distances are read in one unrolled burst (independent LDS loads, then a compare chain in registers); the indices are read
// only when the largest d2 occurs twice — exact duplicates among the rows —, in a second pass.  A rescan stalls its whole wave,
// and early on some lane of the wave inserts at nearly every row: this burst is what the search's time is made of at k = 64.
template <int K, int CANDS>
__device__ __forceinline__ void nn_rescan(const double* ld2, const int* lidx, const int t, double& wd2, int& wslot) {
  wd2 = ld2[t]; wslot = 0;
  bool tie = false;
#pragma unroll
  for (int s = 1; s < K; ++s) {
    const double v = ld2[s * CANDS + t];
    tie = v > wd2 ? false : (v == wd2 ? true : tie);
    wslot = v > wd2 ? s : wslot;
    wd2 = v > wd2 ? v : wd2;
  }
  if (tie) {
    int widx = -1;
    for (int s = 0; s < K; ++s) {
      const int ii = lidx[s * CANDS + t];
      if (ld2[s * CANDS + t] == wd2 && ii > widx) { widx = ii; wslot = s; }
    }
  }
}

struct NnSearchArgs {
  const double* Xs;      // [Np][DP] scaled rows, zero from N on
  const double* Ps;      // [Mp][DP] scaled candidates
  int* nbr;              // [M][K]
  int64_t M;
  int N;
};

template <int DP, int K>
__global__ __launch_bounds__(nn_search_cands(K)) void nn_search_kernel(const NnSearchArgs a) {
  constexpr int CANDS = nn_search_cands(K);
  extern __shared__ __attribute__((aligned(16))) double nn_lds[];
  double* ld2 = nn_lds;                                   // [K][CANDS]
  double* xs = nn_lds + K * CANDS;                        // [NN_CHUNK][DP]
  int* lidx = reinterpret_cast<int*>(xs + NN_CHUNK * DP);   // [K][CANDS]
  const int t = threadIdx.x;
  const int64_t m = (int64_t)blockIdx.x * CANDS + t;
  double xc[DP];
  nn_load_row<DP>(a.Ps, m < a.M ? m : a.M - 1, xc);
  bool nanc = false;
#pragma unroll
  for (int u = 0; u < DP; ++u) nanc = nanc || (xc[u] != xc[u]);
  // the first K rows fill the list
  for (int s = 0; s < K; ++s) {
    const double* xr = a.Xs + (int64_t)s * DP;
    double d2 = 0.0;
#pragma unroll
    for (int u = 0; u < DP; ++u) {
      const double df = xc[u] - xr[u];
      d2 = fma(df, df, d2);
    }
    ld2[s * CANDS + t] = d2;
    lidx[s * CANDS + t] = s;
  }
  double wd2;
  int wslot;
  nn_rescan<K, CANDS>(ld2, lidx, t, wd2, wslot);
  for (int base = K; base < a.N; base += NN_CHUNK) {
    __syncthreads();      // everyone is done with the previous chunk
    {
      const double2* src = reinterpret_cast<const double2*>(a.Xs + (int64_t)base * DP);
      double2* dst = reinterpret_cast<double2*>(xs);
      for (int e = t; e < NN_CHUNK * DP / 2; e += CANDS) dst[e] = src[e];
    }
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < NN_CHUNK; r += 2) {
      const double* xr = xs + r * DP;      // the same address in every lane: LDS broadcast
      double d2a = 0.0, d2b = 0.0;
#pragma unroll
      for (int u = 0; u < DP; ++u) {
        const double da = xc[u] - xr[u], db = xc[u] - xr[DP + u];
        d2a = fma(da, da, d2a);
        d2b = fma(db, db, d2b);
      }
      const int i = base + r;
      if (i < a.N && d2a < wd2) {
        ld2[wslot * CANDS + t] = d2a;
        lidx[wslot * CANDS + t] = i;
        nn_rescan<K, CANDS>(ld2, lidx, t, wd2, wslot);
      }
      if (i + 1 < a.N && d2b < wd2) {
        ld2[wslot * CANDS + t] = d2b;
        lidx[wslot * CANDS + t] = i + 1;
        nn_rescan<K, CANDS>(ld2, lidx, t, wd2, wslot);
      }
    }
  }
  // the list in (d2, index) order: selection sort over the lane's own slots
  for (int s = 0; s < K - 1; ++s) {
    double bd2 = ld2[s * CANDS + t];
    int bidx = lidx[s * CANDS + t], bslot = s;
    for (int q = s + 1; q < K; ++q) {
      const double v = ld2[q * CANDS + t];
      const int ii = lidx[q * CANDS + t];
      if (v < bd2 || (v == bd2 && ii < bidx)) { bd2 = v; bidx = ii; bslot = q; }
    }
    if (bslot != s) {
      ld2[bslot * CANDS + t] = ld2[s * CANDS + t];
      lidx[bslot * CANDS + t] = lidx[s * CANDS + t];
      ld2[s * CANDS + t] = bd2;
      lidx[s * CANDS + t] = bidx;
    }
  }
  if (m >= a.M) return;
  int* out = a.nbr + m * K;
  for (int s = 0; s < K; ++s) out[s] = nanc ? -1 : lidx[s * CANDS + t];
}

struct NnSolveArgs {
  const double* Xs;      // [Np][DP]
  const double* y;       // [N]
  const double* Ps;      // [Mp][DP]
  const int* nbr;        // [M][K], sorted; -1: a candidate with a NaN coordinate
  double* mu;
  double* sd;
  double* ys;
  int64_t M;
  double amplitude, diag, y_mean, y_std;
  int acq;
  double param, y_max;
};

// -acq(mean, sd): acq_value's expressions (acq_kernels.hip) without constraints
__device__ __forceinline__ double nn_acq_value(const int acq, const double param, const double y_max, const double mean, const double sd) {
  double base;
  if (acq == GPBO_ACQ_UCB) {
    base = mean + param * sd;
  } else {
    const double aa = mean - y_max - param;
    const double z = aa / sd;
    if (acq == GPBO_ACQ_EI) base = aa * ndtr_dev(z) + sd * norm_pdf_dev(z);
    else if (acq == GPBO_ACQ_POI) base = ndtr_dev(z);
    else base = log_ei_dev(aa, sd);
  }
  return -1.0 * base;
}

template <int DP, int KERNEL, int K>
__global__ __launch_bounds__(64 * NN_SOLVE_WAVES) void nn_solve_kernel(const NnSolveArgs a) {
  constexpr int PACK = nn_solve_pack(K), P = K + 1, SLOTS = NN_SOLVE_WAVES * PACK;
  extern __shared__ __attribute__((aligned(16))) double nn_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int sub = lane / K, row = lane % K;
  const int slot = wave * PACK + sub;
  const int64_t m = (int64_t)blockIdx.x * SLOTS + slot;
  const bool live = m < a.M;
  const int64_t mm = live ? m : a.M - 1;
  double* A = nn_lds + slot * (K * P);                      // [K][P], the lower triangle
  double* rb = nn_lds + SLOTS * (K * P) + slot * DP;        // the broadcast line; the second buffer SLOTS * DP further
  const int nb = a.nbr[mm * K + row];
  int fail = nb < 0 ? 1 : 0;
  const int idx = nb < 0 ? 0 : nb;
  double xr[DP];
  nn_load_row<DP>(a.Xs, idx, xr);
  double u = a.y[idx];
  double v;
  {
    const double* xc = a.Ps + mm * DP;      // the same address in every lane of the candidate
    double d2 = 0.0;
#pragma unroll
    for (int t = 0; t < DP; ++t) {
      const double df = xc[t] - xr[t];
      d2 = fma(df, df, d2);
    }
    v = a.amplitude * gpbo_kernel_value<KERNEL>(d2);
  }
  // A: the rows take turns through the broadcast line
  if (row == 0) {
#pragma unroll
    for (int t = 0; t < DP; ++t) rb[t] = xr[t];
  }
  nn_wave_sync();
  for (int j = 0; j < K; ++j) {
    const double* cur = rb + (j & 1) * (SLOTS * DP);
    double* nxt = rb + ((j + 1) & 1) * (SLOTS * DP);
    if (row == j + 1) {
#pragma unroll
      for (int t = 0; t < DP; ++t) nxt[t] = xr[t];
    }
    double d2 = 0.0;
#pragma unroll
    for (int t = 0; t < DP; ++t) {
      const double df = xr[t] - cur[t];
      d2 = fma(df, df, d2);
    }
    const double kv = a.amplitude * gpbo_kernel_value<KERNEL>(d2);
    if (row >= j) A[row * P + j] = (row == j) ? a.diag : kv;
    nn_wave_sync();      // row j + 1 is in the line; every lane is done with row j
  }
  // L = chol(A), right-looking, with u = L^-1 y_nn and v = L^-1 k* in the same sweep
  for (int j = 0; j < K; ++j) {
    const double piv = A[j * P + j];      // the same address in every lane of the candidate
    if (!(piv > 0.0)) fail = 1;
    const double ljj = sqrt(piv);
    const double lij = row > j ? A[row * P + j] / ljj : 0.0;
    if (row > j) A[row * P + j] = lij;
    const double zu = __shfl(u, sub * K + j) / ljj, zv = __shfl(v, sub * K + j) / ljj;
    if (row == j) {
      u = zu;
      v = zv;
    } else if (row > j) {
      u = fma(-lij, zu, u);
      v = fma(-lij, zv, v);
    }
    nn_wave_sync();      // column j is whole
    for (int b = j + 1; b < K; ++b) {
      if (b <= row) A[row * P + b] = fma(-lij, A[b * P + j], A[row * P + b]);
    }
    nn_wave_sync();      // the trailing triangle is updated: the next pivot is final
  }
  double q = v * v, dt = v * u;
#pragma unroll
  for (int off = 1; off < K; off <<= 1) {
    q = q + __shfl_xor(q, off);
    dt = dt + __shfl_xor(dt, off);
    fail |= __shfl_xor(fail, off);
  }
  if (row != 0 || !live) return;
  const double var = a.amplitude - q;
  double mean, sd, val;
  if (fail || var != var) {
    mean = sd = val = __builtin_nan("");
  } else {
    mean = a.y_mean + a.y_std * dt;
    sd = a.y_std * sqrt(var > 0.0 ? var : 0.0);
    val = nn_acq_value(a.acq, a.param, a.y_max, mean, sd);
  }
  a.mu[m] = mean;
  a.sd[m] = sd;
  a.ys[m] = val;
}

template <typename F>
static int with_nn_k(gpbo_ctx* ctx, int k, F&& f) {
  switch (k) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
  }
  GPBO_FAIL(ctx, GPBO_ERR_INVALID, "nn_acq_argbest: k must be 16, 32 or 64");
}

int launch_nn_values(gpbo_ctx* ctx, const NnCall& c) {
  const int d = c.d, DP = pad_dim(d), k = c.k;
  const int64_t N = c.N, M = ctx->M;
  const NnBlock b = nn_block(N, d, DP, M, k);
  int rc;
  if ((rc = ensure(ctx, &ctx->nn, &ctx->cap_nn, b.doubles))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  double* ws = ctx->nn;
  // stage 0: upload and scaling
  jes_mark(ctx, ctx->nn_clock, 0);
  GPBO_HIP(ctx, hipMemcpyAsync(ws + b.ls, c.ls, 64 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(ws + b.raw, c.X, (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(ws + b.y, c.y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = launch_prescale(ctx, ws + b.raw, N, d, DP, ws + b.ls, ws + b.Xs, b.Np))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, ws + b.ls, ws + b.Ps, b.Mp))) return rc;
  // the pageable sources above are the caller's: they are read before the call returns (the selection synchronises)
  int* nbr = reinterpret_cast<int*>(ws + b.nbr);
  // stage 1: the neighbour search
  jes_mark(ctx, ctx->nn_clock, 1);
  NnSearchArgs s{};
  s.Xs = ws + b.Xs; s.Ps = ws + b.Ps; s.nbr = nbr; s.M = M; s.N = (int)N;
  rc = with_nn_k(ctx, k, [&](auto kk) -> int {
    constexpr int K = decltype(kk)::value;
    const int64_t blocks = (M + nn_search_cands(K) - 1) / nn_search_cands(K);
    switch (DP) {
#define NN_SEARCH_CASE(W)                                                                                                              \
  case W: {                                                                                                                            \
    const int lds = (int)nn_search_lds(K, W);                                                                                          \
    GPBO_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(nn_search_kernel<W, K>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                      lds));                                                                                           \
    nn_search_kernel<W, K><<<dim3((unsigned)blocks), dim3(nn_search_cands(K)), lds, ctx->stream>>>(s);                                 \
    break;                                                                                                                             \
  }
      NN_SEARCH_CASE(4) NN_SEARCH_CASE(8) NN_SEARCH_CASE(16) NN_SEARCH_CASE(32) NN_SEARCH_CASE(64)
#undef NN_SEARCH_CASE
      default: GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "nn_acq_argbest: unsupported padded dimension");
    }
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
  if (rc) return rc;
  // stage 2: the local solves
  jes_mark(ctx, ctx->nn_clock, 2);
  NnSolveArgs v{};
  v.Xs = ws + b.Xs; v.y = ws + b.y; v.Ps = ws + b.Ps; v.nbr = nbr; v.mu = ws + b.mu; v.sd = ws + b.sd; v.ys = ctx->ys; v.M = M;
  v.amplitude = c.amplitude; v.diag = c.amplitude + (c.amplitude * c.white + c.alpha); v.y_mean = c.y_mean; v.y_std = c.y_std;
  v.acq = c.acq; v.param = c.param; v.y_max = c.y_max;
  rc = with_nn_k(ctx, k, [&](auto kk) -> int {
    constexpr int K = decltype(kk)::value;
    const int64_t blocks = (M + nn_solve_cands(K) - 1) / nn_solve_cands(K);
    return with_dp_kernel(ctx, DP, c.kernel, [&](auto dp, auto kind) -> int {
      constexpr int W = decltype(dp)::value;
      const int lds = (int)nn_solve_lds(K, W);
      const void* fn = reinterpret_cast<const void*>(nn_solve_kernel<W, decltype(kind)::value, K>);
      GPBO_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      nn_solve_kernel<W, decltype(kind)::value, K><<<dim3((unsigned)blocks), dim3(64 * NN_SOLVE_WAVES), lds, ctx->stream>>>(v);
      GPBO_HIP(ctx, hipGetLastError());
      return GPBO_OK;
    });
  });
  if (rc) return rc;
  jes_mark(ctx, ctx->nn_clock, 3);      // stage 3, the selection, is the caller's; it records event 4 behind it (nn_mark_end)
  return GPBO_OK;
}

void nn_mark_end(gpbo_ctx* ctx) { jes_mark(ctx, ctx->nn_clock, 4); }

}  // namespace gpbo
