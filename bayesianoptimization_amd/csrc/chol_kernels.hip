// Blocked Cholesky, round-3 schedule (gfx950): 128-column steps inside 512-column outer panels.
//
// What it replaces: cholesky(K, lower=True) -> LAPACK dpotrf   (sklearn _gpr.py:349, via scipy.linalg.cholesky)
//
// Why 128: the factorisation is a latency chain, not a flop problem (round 2: 0.68 us per column at every N, the
// matrix pipe 2-5 % busy on the chain kernels).  fp64 runs at 32 flop/clk/SIMD on VALU and MFMA alike, so ONE compute
// unit needs 1.7 us for a 64^3 product: whatever sits on the chain must be small, and everything else must be wide.
// Per 128 columns the chain is now
//     diagonal block (ONE workgroup, no launch inside: potf2 of 128x64 -> SYRK -> potf2 of 64x64 -> the two 64x64 inverses)
//  -> panel solve of ALL rows below (16 rows per workgroup, three chained 16-row MFMA products, no explicit 128x128 inverse)
//  -> rank-128 update of the NEXT diagonal block only (36 small workgroups)
//  -> [next diagonal block || rest of the in-panel update] in one launch
// i.e. three launches per 128 columns where round 2 had two per 64, and the diagonal workgroup no longer applies the
// previous column block's update to its own block by itself (that 64^3 product cost 1.7 us per step on one CU; for a
// 128-block it would be 8.5 us).  The rank-512 trailing update per outer panel is unchanged (gemm128_f64_kernel).
//
// Every kernel here takes a lane index (blockIdx.y / .z) so that gpbo_lml_batch's theta lanes share the launches.
#include <cstdlib>

#include "chol_bodies.h"
#include "fit_bodies.h"

namespace gpbo {

// One launch = diagonal block(s) kb (workgroup 0) || the 64x64 tiles of the previous column block's in-panel update, two per
// 512-thread workgroup (every tile but the leading skip00 x skip00 ones, which chol128_diag_update_kernel has already
// brought up to date).
// (waves_per_eu(2, 2): the launch's dynamic LDS gives every workgroup a CU to itself, so 256 VGPRs are there for the taking — 156 used)
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void chol128_step_kernel(double* L, int64_t ld, int kb, int nblk, double* dinv, int* info,
                                                            GemmArgs g, int tiles_n, int tiles, int64_t lane_stride, long long* stamps) {
  extern __shared__ __attribute__((aligned(16))) double c128_smem[];
  const int zl = (int)blockIdx.y;
  if (blockIdx.x == 0) {
    diag128_body(L + (int64_t)zl * lane_stride, ld, kb, nblk, dinv + (int64_t)zl * lane_stride, info + (int64_t)zl * lane_stride * 2,
                 c128_smem, stamps, (int)threadIdx.x);
    return;
  }
  const int half = (int)(threadIdx.x >> 8);
  const int t = 2 * ((int)blockIdx.x - 1) + half;
  // LIVE tiles only (round 6), in the order [lower triangle of the leading tiles_n x tiles_n tiles, by rows | the full rows below it],
  // the leading skip00 (skip00 + 1) / 2 of which belong to chol128_diag_update_kernel.  The square grid's dead upper tiles were
  // not free: a dead tile goes through the loads and barriers of a live one beside its partner half, so a one-panel factorisation
  // (NP <= 2048) ran twice the workgroups it needed — 392 for 203 live pairs at the second step of N = 2048: two rounds over the
  // chip's 256 CUs (the launch's dynamic LDS admits one workgroup per CU), 39 us against the diagonal workgroup's 23.
  const int tt = t + g.skip00 * (g.skip00 + 1) / 2;
  const int tri = tiles_n * (tiles_n + 1) / 2;
  int bm, bn;
  if (tt < tri) lower_tile_of(tt, bm, bn);
  else { bm = tiles_n + (tt - tri) / tiles_n; bn = (tt - tri) - (bm - tiles_n) * tiles_n; }
  const bool mine = t < tiles;
  if (!mine) { bm = g.m / 64 - 1; bn = 0; }   // a tile that exists (the last row tile): loads only, same barrier count
  GemmArgs h = g;
  h.lower_only = 0; h.skip00 = 0;            // decided above
  gemm_tile_body<true, false>(h, bm, bn, zl, 0, c128_smem + half * GT_LDS_DOUBLES, (int)(threadIdx.x & 255), mine);
}

// Panel solve below a 128-column diagonal block (16 rows per workgroup) and the rank-128 update of the NEXT diagonal block (one
// 16x16 tile per workgroup): the bodies live in chol_bodies.h (the fused small-problem kernel runs them too).
__global__ __launch_bounds__(256) void chol128_panel_kernel(double* L, int64_t ld, int kb, const double* __restrict__ dinv,
                                                             int64_t lane_stride) {
  __shared__ __attribute__((aligned(16))) double XT[C128_PANEL_LDS_DOUBLES];
  chol128_panel_body(L + (int64_t)blockIdx.y * lane_stride, ld, kb, dinv + (int64_t)blockIdx.y * lane_stride, (int)blockIdx.x, XT,
                     (int)threadIdx.x);
}

__global__ __launch_bounds__(256) void chol128_diag_update_kernel(double* L, int64_t ld, int kb, int64_t lane_stride) {
  __shared__ __attribute__((aligned(16))) double Ps[C128_UPD_LDS_DOUBLES];
  chol128_diag_update_body(L + (int64_t)blockIdx.y * lane_stride, ld, kb, (int)blockIdx.x, Ps, (int)threadIdx.x);
}

// ---- launchers -------------------------------------------------------------------------------------------------------
static int launch_step(gpbo_ctx* ctx, Model& m, int kb, int nblk, const GemmArgs* upd, long long* stamps) {
  if (!(ctx->func_attrs & ATTR_CHOL128)) {
    GPBO_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(chol128_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)C128_LDS_BYTES));
    ctx->func_attrs |= ATTR_CHOL128;
  }
  GemmArgs g{};
  int tiles = 0, tiles_n = 1;
  if (upd) {
    g = *upd;
    g.lanes = ctx->lanes; g.lane_stride = ctx->lane_stride; g.batch = 1;
    tiles_n = g.n / 64;
    const int tiles_m = g.m / 64;
    if (!g.lower_only || tiles_m < tiles_n) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "cholesky128: the step's update must be lower-only with m >= n");
    // live tiles: the lower triangle of the leading tiles_n rows + the full rows below, less the leading skip00-block's
    tiles = tiles_n * (tiles_n + 1) / 2 + (tiles_m - tiles_n) * tiles_n - g.skip00 * (g.skip00 + 1) / 2;
    if (tiles_m <= g.skip00 && tiles_n <= g.skip00) tiles = 0;   // nothing but the block the diagonal workgroup owns
  }
  chol128_step_kernel<<<dim3((unsigned)(1 + (tiles + 1) / 2), (unsigned)ctx->lanes), dim3(512), C128_LDS_BYTES, ctx->stream>>>(
      m.L, m.NP, kb, nblk, m.dinv, ctx->info_dev, g, tiles_n, tiles, ctx->lane_stride, stamps);
  GPBO_HIP(ctx, hipGetLastError());
  return GPBO_OK;
}

// ---- look-ahead over the outer panels ----------------------------------------------------------------------------
// The rank-`outer` trailing update of panel p only has to reach the NEXT panel's columns before that panel's chain can
// start; the rest of it (T_b) is independent of the chain and runs on a second ("bulk") stream meanwhile:
//     main:  chain(p) | [wait T_b(p-1)] T_a(p) | chain(p+1) | ...
//     bulk:                             [wait T_a(p)] T_b(p)
// (T_b starts behind T_a, not beside it: side by side the two share the chip and T_a, which the chain waits for, takes
// 106 us instead of ~45 at N = 4096)
// T_a(p) waits for T_b(p-1) because both accumulate into the next panel's columns and the order of the two rank-512
// contributions is part of the result (bitwise the one-stream factor: same launches, same kernels, same order per tile).
// Round 2 measured this with a plain second stream and dropped it: the bulk GEMM's workgroups hold every CU, so the
// chain's small kernels queue behind them.  Round 3 measured a bulk stream confined to a subset of the CUs
// (hipExtStreamCreateWithCUMask, 128 to 224 of 256) within noise of the plain one, which is what is used.
// GPBO_CHOL_LA=0 turns the look-ahead off (A/B runs).
static int lookahead_min_np() {
  static const int v = [] {
    const char* e = dbg_env("GPBO_CHOL_LA");
    if (e && e[0] == '0') return 1 << 30;
    const char* f = dbg_env("GPBO_CHOL_LA_MIN_NP");
    return f ? atoi(f) : 4096;     // measured (scripts/archive/r03_la_probe.py): 2048 0.709 -> 0.721 ms, 4096 1.82 -> 1.75, 8192 6.42 -> 6.17
  }();
  return v;
}

static LookAhead* lookahead_for(gpbo_ctx* ctx, int n_events) {
  LookAhead* la = nullptr;
  for (auto& l : ctx->lookahead)
    if (l.main == ctx->stream) la = &l;
  if (!la) {
    LookAhead l;
    l.main = ctx->stream;
    if (hipStreamCreateWithFlags(&l.bulk, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    ctx->lookahead.push_back(l);
    la = &ctx->lookahead.back();
  }
  while ((int)la->ev.size() < n_events) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    la->ev.push_back(ev);
  }
  return la;
}

// Blocked Cholesky of m.L (lower, in place), inverted 64x64 diagonal blocks to m.dinv: 128-column steps inside
// `outer`-column panels (outer a multiple of 128), one rank-`outer` trailing update per panel.
int launch_cholesky128(gpbo_ctx* ctx, Model& m, int outer, long long* stamps) {
  const int nblk = (int)(m.NP / NB);
  const int per_outer = outer / NB;
  const unsigned lanes = (unsigned)ctx->lanes;
  int rc;
  const int n_panels = (nblk + per_outer - 1) / per_outer;
  LookAhead* la = (ctx->lanes == 1 && !ctx->no_lookahead && m.NP >= lookahead_min_np() && n_panels >= 3) ? lookahead_for(ctx, 2 * n_panels) : nullptr;
  bool la_joined = true;
  int pidx = 0;     // outer panel index
  for (int ob = 0; ob < nblk; ob += per_outer) {
    const int oe = (ob + per_outer < nblk) ? ob + per_outer : nblk;
    if ((rc = launch_step(ctx, m, ob, (oe - ob >= 2) ? 2 : 1, nullptr, stamps))) return rc;   // everything before the panel is applied
    for (int kb = ob; kb < oe; kb += 2) {
      const int wb = (oe - kb >= 2) ? 2 : 1;
      const int rem = (int)(m.NP - (int64_t)(kb + wb) * NB);      // rows below the diagonal block
      if (rem == 0) break;
      if (wb != 2) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "cholesky128: a single 64-block can only end the matrix");
      chol128_panel_kernel<<<dim3((unsigned)(rem / 16), lanes), dim3(256), 0, ctx->stream>>>(m.L, m.NP, kb, m.dinv, ctx->lane_stride);
      GPBO_HIP(ctx, hipGetLastError());
      const int next = kb + 2;
      if (next < oe) {
        const int nb2 = (oe - next >= 2) ? 2 : 1;
        const int nt = 4 * nb2;
        chol128_diag_update_kernel<<<dim3((unsigned)(nt * (nt + 1) / 2), lanes), dim3(256), 0, ctx->stream>>>(m.L, m.NP, kb,
                                                                                                            ctx->lane_stride);
        GPBO_HIP(ctx, hipGetLastError());
        double* panel = m.L + (int64_t)next * NB * m.NP + (int64_t)kb * NB;
        GemmArgs s{};    // rank-128 update of the panel's remaining columns; the next diagonal block is already done
        s.m = rem; s.n = (oe - next) * NB; s.k = 2 * NB; s.alpha = -1.0; s.beta = 1.0;
        s.A = panel; s.lda = m.NP; s.B = panel; s.ldb = m.NP; s.b_trans = 1;
        s.C = m.L + (int64_t)next * NB * m.NP + (int64_t)next * NB; s.ldc = m.NP;
        s.lower_only = 1; s.skip00 = nb2;
        if ((rc = launch_step(ctx, m, next, nb2, &s, nullptr))) return rc;
      }
    }
    const int rem2 = (int)(m.NP - (int64_t)oe * NB);
    if (rem2 > 0) {
      const double* P = m.L + (int64_t)oe * NB * m.NP + (int64_t)ob * NB;
      GemmArgs t{};
      t.k = (oe - ob) * NB; t.alpha = -1.0; t.beta = 1.0;
      t.lda = m.NP; t.ldb = m.NP; t.b_trans = 1; t.ldc = m.NP;
      t.batch = 1; t.lower_only = 1;
      // one decision for the whole update, whichever way it is launched below (whole, or the next panel's columns + the rest): the
      // sixteen-wave tile kernel sums k in another order, and L must not depend on the look-ahead
      t.m = rem2; t.n = rem2;
      t.fat = gemm_fat_rule(t) ? 1 : -1;
      const int nw = rem2 < outer ? rem2 : outer;       // the next panel's columns
      if (!la || rem2 <= nw) {
        if (la && pidx > 0) GPBO_HIP(ctx, hipStreamWaitEvent(ctx->stream, la->ev[2 * (pidx - 1) + 1], 0));
        t.m = rem2; t.n = rem2; t.A = P; t.B = P;
        t.C = m.L + (int64_t)oe * NB * m.NP + (int64_t)oe * NB;
        if ((rc = launch_gemm(ctx, t))) return rc;
        la_joined = true;
      } else {
        if (pidx > 0) GPBO_HIP(ctx, hipStreamWaitEvent(ctx->stream, la->ev[2 * (pidx - 1) + 1], 0));
        t.m = rem2; t.n = nw; t.A = P; t.B = P;
        t.C = m.L + (int64_t)oe * NB * m.NP + (int64_t)oe * NB;
        if ((rc = launch_gemm(ctx, t))) return rc;        // T_a on main, with the whole chip to itself:
        GPBO_HIP(ctx, hipEventRecord(la->ev[2 * pidx], ctx->stream));   // the bulk stream starts behind it
        hipStream_t main_stream = ctx->stream;
        ctx->stream = la->bulk;
        hipError_t e = hipStreamWaitEvent(la->bulk, la->ev[2 * pidx], 0);
        if (e == hipSuccess) {
          t.m = rem2 - nw; t.n = rem2 - nw; t.A = P + (int64_t)nw * m.NP; t.B = t.A;
          t.C = m.L + ((int64_t)oe * NB + nw) * m.NP + ((int64_t)oe * NB + nw);
          rc = launch_gemm(ctx, t);                          // T_b on bulk
          if (rc == GPBO_OK) e = hipEventRecord(la->ev[2 * pidx + 1], la->bulk);
        }
        ctx->stream = main_stream;
        if (rc) return rc;
        GPBO_HIP(ctx, e);
        la_joined = false;
      }
    }
    ++pidx;
  }
  // nothing of the factorisation may still be in flight on the bulk stream when main goes on (it always joined above:
  // the last update has no far part)
  if (la && !la_joined && pidx > 0) GPBO_HIP(ctx, hipStreamWaitEvent(ctx->stream, la->ev[2 * (pidx - 1) + 1], 0));
  return GPBO_OK;
}

}  // namespace gpbo
