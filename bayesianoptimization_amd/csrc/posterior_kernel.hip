// Posterior launcher + finalize kernel (gfx950).
//
// gpbo_posterior replaces, per candidate (SK = sklearn/gaussian_process):
//   K_trans = kernel_(X, X_train_)                     SK/_gpr.py:443   (Matern/RBF: kernels.py:1715-1724, 1556-1565)
//   y_mean  = K_trans @ alpha_                         SK/_gpr.py:444-447
//   V       = solve_triangular(L_, K_trans.T)          SK/_gpr.py:454-456   -> here V = W k*, W = L^-1
//   y_var   = 1 - einsum("ij,ji->i", V.T, V); clip; * y_std^2; sqrt      SK/_gpr.py:474-494
// and dispatches to one of six device paths (PostPath; the rule and its measurements: posterior_plan.h):
//   Small      posterior_small.hip      batched GEMV (latency path: predicts of the host optimisers)
//   Fused256   posterior_kernel_v2.hip  GEN = 1: k* generated inside the MFMA kernel, 8 waves, 256-row chunks
//   Fused512   posterior_kernel_v2.hip  GEN = 1, 16 waves, 512-row chunks
// and the three slab paths, which share one walk (launch_posterior_slabs below; the slab's size and caps: slab_spec,
// posterior_plan.h) and one k* generator (kstar_gen_kernel<.., the path>, posterior_kernel_v2.hip) and differ in their GEMM:
//   SlabF64    posterior_kernel_v2.hip  GEN = 2: k* slab generated once + fp64 MFMA GEMM
//   SlabI8     posterior_i8.hip         the same slab as int8 digit planes + int8 MFMA GEMM
//   SlabF32    posterior_kernel_f32.hip fp32 k* slab + fp32 MFMA GEMM (precision F32)
// The row-chunk partial sums every path but Small writes are combined in a fixed order by posterior_finalize_kernel (a fused
// kernel whose workgroups hold all rows of their candidates does it itself), so results are run-to-run deterministic.  (The
// first version of the fused kernel — 128 candidates x 256 rows per workgroup, 2 waves/SIMD, 403 ms per C3 launch — is in the
// git history; docs/LAB_NOTEBOOK.md §4.1.)
#include <algorithm>
#include <cstdlib>

#include "gpbo_internal.h"
#include "fit_bodies.h"
#include "i8_digits.h"

namespace gpbo {

typedef double d4 __attribute__((ext_vector_type(4)));

// mu = y_std * (k* . alpha) + y_mean ; sd = sqrt(max(c (1 - sum_chunks part) + white, 0) * y_std^2)
// NAN_FROM_MU (the int8 GEMM's partials): its sum of squares comes from the integer digits of k*, and an integer cannot carry a NaN
// (a NaN k* quantises to some integer): sd would come out finite where the fp64 paths and sklearn give NaN.  The partial means are
// fp64 sums over the same k*, NaN exactly when one of them is, so sd takes mu's NaN.  Finite candidates keep the bits of the plain
// instance: one chunk-sum order for both.
template <bool NAN_FROM_MU>
__global__ __launch_bounds__(256) void posterior_finalize_kernel(const double* __restrict__ part,
                                                                 const double* __restrict__ mu_part,
                                                                 int nchunks, int n_mu, int64_t Mp, int64_t M,
                                                                 double y_mean, double y_std, double amplitude, double white,
                                                                 double* __restrict__ mu,
                                                                 double* __restrict__ sd, int* __restrict__ negvar) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  double ss = 0.0;
  for (int r = 0; r < nchunks; ++r) ss += part[(int64_t)r * Mp + m];
  double mun = 0.0;
  for (int q = 0; q < n_mu; ++q) mun += mu_part[(int64_t)q * Mp + m];
  if (NAN_FROM_MU && mun != mun) ss = mun;
  posterior_finalize_elem(ss, mun, y_mean, y_std, amplitude, white, mu + m, sd + m, negvar);
}

// Candidates per k* slab: what the workspace budget holds at bytes_per_cand — GPBO_KSTAR_GB (default 4 GB), clipped to 80 % of
// what the device could give the slab; hipMemGetInfo is asked only when the slab buffer would have to grow (it costs tens of
// microseconds per call) — and at most `cap`, rounded down to 128, at most Mp.  Below 128 the walk decides.
static int64_t kstar_slab_width(gpbo_ctx* ctx, int64_t Mp, int64_t bytes_per_cand, int64_t cap) {
  const char* e = getenv("GPBO_KSTAR_GB");      // read per call: the slab-loop test changes it between passes
  const double budget_gb = (e && atof(e) > 0.0) ? atof(e) : 4.0;
  int64_t budget = (int64_t)(budget_gb * 1e9);
  const int64_t want = Mp * bytes_per_cand < budget ? Mp * bytes_per_cand : budget;
  if (want > ctx->cap_kst * 8) {                 // the buffer we hold is too small: what could the device give?
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const int64_t avail = (int64_t)(((double)free_b + (double)ctx->cap_kst * 8.0) * 0.8);
      if (avail < budget) budget = avail;
    }
  }
  const int64_t ms = std::min(budget / bytes_per_cand, cap) / 128 * 128;
  return std::min(ms, Mp);
}

// The slab paths: the candidates in slabs of ms, per slab the k* generation into ctx->kst (+ the partial means) and the path's GEMM
// over it (the partial sums of squares).  The int8 path first makes sure of W's digit planes (prepare_posterior_i8).
static int launch_posterior_slabs(gpbo_ctx* ctx, Model& m, int64_t Mp, const PostPlan& plan) {
  int rc;
  if (plan.path == PostPath::SlabI8 && (rc = prepare_posterior_i8(ctx, m))) return rc;
  const SlabSpec spec = slab_spec(plan.path, m.NP);
  int64_t ms = kstar_slab_width(ctx, Mp, spec.bytes_per_cand, spec.offset_cap);
  if (plan.path == PostPath::SlabI8) ms = i8_slab_width(m.NP, spec.bytes_per_cand, ms, ctx->compute_units);
  if (ms < 128) {
    if (!spec.narrow_ok) GPBO_FAIL(ctx, GPBO_ERR_HIP, "posterior: not enough device memory for one k* slab");
    ms = 128;
  }
  if ((rc = ensure(ctx, &ctx->kst, &ctx->cap_kst, slab_doubles(ms, spec.bytes_per_cand)))) return rc;
  if (ms / 64 * plan.part_chunks > 0x7fffffffLL)   // the GEMM's grid for a full slab: 64-candidate tiles x row chunks
    GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "posterior: grid too large; shard the candidates");
  for (int64_t m0 = 0; m0 < Mp; m0 += ms) {
    const int64_t ldk = std::min(ms, Mp - m0);
    switch (plan.path) {
      case PostPath::SlabF64:
        if ((rc = launch_kstar_slab(ctx, m, ctx->kst, ldk, Mp, m0, plan.mu_chunks))) return rc;
        if ((rc = launch_slab_gemm_f64(ctx, m, ctx->kst, ldk, m0, Mp, plan.part_chunks))) return rc;
        break;
      case PostPath::SlabF32:
        if ((rc = launch_kstar_slab_f32(ctx, m, reinterpret_cast<float*>(ctx->kst), ldk, Mp, m0, plan.mu_chunks))) return rc;
        if ((rc = launch_slab_gemm_f32(ctx, m, reinterpret_cast<const float*>(ctx->kst), ldk, m0, Mp, plan.part_chunks))) return rc;
        break;
      case PostPath::SlabI8:
        if ((rc = launch_kstar_digits(ctx, m, ctx->kst, ldk, Mp, m0, plan.mu_chunks))) return rc;
        if ((rc = launch_slab_gemm_i8(ctx, m, ctx->kst, ldk, m0, Mp, plan.part_chunks))) return rc;
        break;
      default: GPBO_FAIL(ctx, GPBO_ERR_STATE, "posterior: not a slab path");
    }
  }
  return GPBO_OK;
}

static int ensure_posterior_outputs(gpbo_ctx* ctx, Model& m, int64_t Mp) {
  if (Mp > m.cap_M) {
    if (m.mu) { GPBO_HIP(ctx, hipFree(m.mu)); m.mu = nullptr; }
    if (m.sd) { GPBO_HIP(ctx, hipFree(m.sd)); m.sd = nullptr; }
    m.cap_M = 0;
    GPBO_HIP(ctx, hipMalloc((void**)&m.mu, (size_t)Mp * sizeof(double)));
    GPBO_HIP(ctx, hipMalloc((void**)&m.sd, (size_t)Mp * sizeof(double)));
    m.cap_M = Mp;
  }
  return GPBO_OK;
}

// mu, sd and their gradients in the (raw) inputs for the M resident candidates (M <= 256): posterior_small.hip
int launch_posterior_grad(gpbo_ctx* ctx, Model& m, int64_t M, double y_mean, double y_std, double** dmu_dev, double** dsd_dev,
                          double** packed_dev, const double* xc_in, double* packed_out) {
  const int64_t Mp = round_up(M, POST_CANDS);
  int rc;
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * m.DP))) return rc;
  if ((rc = ensure(ctx, &ctx->mu_part, &ctx->cap_mu_part, std::max<int64_t>((int64_t)2 * M * m.d + 2 * M, Mp)))) return rc;
  if ((rc = ensure_posterior_outputs(ctx, m, Mp))) return rc;
  // xc_in (gpbo_polish_seeds): the round's points in device-visible pinned host memory, read by the scaling kernel itself
  if ((rc = launch_prescale(ctx, xc_in ? xc_in : ctx->Xc, M, m.d, m.DP, m.ls, ctx->Xcs, Mp))) return rc;
  // packed (gpbo_polish_seeds): mu and sd land right behind the gradients, [dmu | dsd | mu | sd], so that one block brings a
  // round's results back — in packed_out (device-visible pinned host memory, written by the last kernel itself) when given,
  // else in ctx->mu_part for the caller to copy; the model's own mu / sd buffers are then NOT written
  const bool packed = packed_dev || packed_out;
  double* base = packed_out ? packed_out : ctx->mu_part;
  *dmu_dev = base;
  *dsd_dev = base + M * m.d;
  double* mu_out = packed ? base + 2 * M * m.d : m.mu;
  double* sd_out = packed ? mu_out + M : m.sd;
  if (packed_dev) *packed_dev = base;
  ev_begin(ctx, T_POST_MAIN);
  rc = launch_posterior_grad_small(ctx, m, (int)M, y_mean, y_std, *dmu_dev, *dsd_dev, mu_out, sd_out);
  ev_end(ctx, T_POST_MAIN);
  if (rc) return rc;
  m.M_post = packed ? -1 : M;
  m.refreshable = false;
  m.N_post = m.N;
  m.ystd_post = y_std;
  return GPBO_OK;
}

// plan -> buffers -> prescale (unless the ends are fused) -> the path's launcher -> finalize (unless the ends are fused or Small)
int launch_posterior(gpbo_ctx* ctx, Model& m, int64_t M, double y_mean, double y_std) {
  const int64_t Mp = round_up(M, POST_CANDS);
  const char* kv = dbg_env("GPBO_POST_KERNEL");      // debug build: A/B switches (posterior_plan.h)
  const char* sm = dbg_env("GPBO_POST_SMALL");
  const char* fe = dbg_env("GPBO_POST_FUSE_ENDS");
  const PostPlan plan = plan_posterior(m.NP, M, m.precision == GPBO_F32, small_batch_limit(m.NP), kv ? kv[0] - '0' : 0,
                                       sm && sm[0] == '0', fe && fe[0] == '0');
  int rc;
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * m.DP))) return rc;
  if (plan.path != PostPath::Small) {   // (the GEMV path sizes its own scratch in ctx->part)
    if ((rc = ensure(ctx, &ctx->part, &ctx->cap_part, (int64_t)plan.part_chunks * Mp))) return rc;
    if ((rc = ensure(ctx, &ctx->mu_part, &ctx->cap_mu_part, (int64_t)plan.mu_chunks * Mp))) return rc;
  }
  if ((rc = ensure_posterior_outputs(ctx, m, Mp))) return rc;
  if (!plan.fuse_ends && (rc = launch_prescale(ctx, ctx->Xc, M, m.d, m.DP, m.ls, ctx->Xcs, Mp))) return rc;
  const PostEnds ends{ctx->Xc, m.ls, m.d, M, y_mean, y_std, m.amplitude, m.white, m.mu, m.sd, ctx->negvar};
  ev_begin(ctx, T_POST_MAIN);
  switch (plan.path) {
    case PostPath::Small: rc = launch_posterior_small(ctx, m, (int)M, y_mean, y_std); break;
    case PostPath::Fused256:
    case PostPath::Fused512: rc = launch_posterior_fused(ctx, m, Mp, plan, ends); break;
    case PostPath::SlabF64:
    case PostPath::SlabI8:
    case PostPath::SlabF32: rc = launch_posterior_slabs(ctx, m, Mp, plan); break;
  }
  ev_end(ctx, T_POST_MAIN);
  if (rc) return rc;
  ev_begin(ctx, T_POST_FINAL);   // recorded on every path, so that last_timings() always has the key
  if (plan.path == PostPath::SlabI8)
    posterior_finalize_kernel<true><<<dim3((unsigned)((M + 255) / 256)), dim3(256), 0, ctx->stream>>>(
        ctx->part, ctx->mu_part, plan.part_chunks, plan.mu_chunks, Mp, M, y_mean, y_std, m.amplitude, m.white, m.mu, m.sd, ctx->negvar);
  else if (!plan.fuse_ends && plan.path != PostPath::Small)
    posterior_finalize_kernel<false><<<dim3((unsigned)((M + 255) / 256)), dim3(256), 0, ctx->stream>>>(
        ctx->part, ctx->mu_part, plan.part_chunks, plan.mu_chunks, Mp, M, y_mean, y_std, m.amplitude, m.white, m.mu, m.sd, ctx->negvar);
  ev_end(ctx, T_POST_FINAL);
  GPBO_HIP(ctx, hipGetLastError());
  m.M_post = M;
  m.refreshable = false;     // gpbo_posterior_refresh: mu / sd now reflect all m.N rows at this y_std
  m.N_post = m.N;
  m.ystd_post = y_std;
  return GPBO_OK;
}

}  // namespace gpbo
