// C-ABI entry points of libgpbo (see include/gpbo.h for the contract and the reference call each
// function replaces).  Host-side orchestration only: every numeric step is a HIP kernel launched
// on the context's stream.
#include <array>
#include <cmath>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "gpbo_internal.h"
#include "scaled_kernel.h"    // a scaled model c * k + white * I as the unit model at noise (white + alpha) / c

namespace gpbo {

static std::mutex g_err_mu;
// hipGraph captures are taken one at a time, process-wide, and not while another context of the process allocates or uploads
// theta-search inputs (shared side): see gpbo_lml_batch.
static std::shared_mutex g_capture_mu;
static std::string g_err;

void set_global_error(const std::string& s) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = s;
}

static int check_slot(gpbo_ctx* ctx, int slot) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (slot < 0 || slot >= GPBO_MAX_MODELS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "slot out of range");
  return GPBO_OK;
}

// m's buffers in the order of fit_plan.h's table (FitBuf, the per-model part)
static std::array<double**, FB_MODEL_COUNT> model_buffers(Model& m) {
  return {&m.ls, &m.Xs, &m.K, &m.L, &m.W, &m.dinv, &m.tmp, &m.yn, &m.tvec, &m.alpha};
}

static void free_model(Model& m) {
  double** ptrs[] = {&m.ls, &m.Xs, &m.K, &m.L, &m.W, &m.Wp, &m.dinv, &m.tmp, &m.yn, &m.tvec, &m.alpha, &m.mu, &m.sd};
  for (double** p : ptrs) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  if (m.Wp32) (void)hipFree(m.Wp32);
  if (m.Wd) (void)hipFree(m.Wd);
  if (m.wscale) (void)hipFree(m.wscale);
  m = Model();
}

static int alloc_model(gpbo_ctx* ctx, Model& m, int64_t NP, int DP) {
  if (NP <= m.cap_NP && DP <= m.cap_DP && m.K) return GPBO_OK;
  double* mu = m.mu; double* sd = m.sd; int64_t cap_M = m.cap_M;   // keep posterior buffers
  m.mu = m.sd = nullptr;
  free_model(m);
  m.mu = mu; m.sd = sd; m.cap_M = cap_M;
  const FitBuffers sizes = fit_buffers(NP, DP);
  const auto buf = model_buffers(m);
  for (int i = 0; i < FB_MODEL_COUNT; ++i) GPBO_HIP(ctx, hipMalloc((void**)buf[i], (size_t)sizes.size[i] * sizeof(double)));
  GPBO_HIP(ctx, hipMalloc((void**)&m.Wp, (size_t)NP * NP * sizeof(double)));
  m.cap_NP = NP;
  m.cap_DP = DP;
  return GPBO_OK;
}

// Blocked Cholesky of m.L (lower, in place) + the inverted 64x64 diagonal blocks (chol_kernels.hip): 128-column steps —
// one workgroup factors and inverts the diagonal block while the rest of the launch applies the previous step's update —
// inside `outer`-column panels; the matrix right of a panel gets ONE rank-`outer` update per panel, so the trailing
// matrix is read and written N / outer times instead of N / 128 times.  (Round 2's 64-column schedules — potrf_diag_kernel /
// chol_step_kernel — were retired in round 4.)
static int cholesky(gpbo_ctx* ctx, Model& m, long long* stamps = nullptr) {
  return launch_cholesky128(ctx, m, chol_outer(m.NP, env_override(dbg_env("GPBO_CHOL_OUTER"))), stamps);
}

// W = L^-1 by recursive doubling from the inverted 64x64 diagonal blocks:
//   [[A,0],[C,B]]^-1 = [[A^-1,0],[-B^-1 C A^-1, B^-1]]  — two batched GEMMs per level.
// `zero_above`: W's strict upper block triangle is zero-filled first (a fit: the posterior pack and gpbo_get_Linv read W as a
// square).  An LML evaluation reads W by tiles at and below the diagonal only — these products, t = W y, alpha = W^T t, W^T W with
// its k-loop cut at the tiles' diagonal — and skips the 8 NP^2-byte fill (18 us + a 6 us gap at N = 4096).
static int trtri(gpbo_ctx* ctx, Model& m, bool zero_above = true) {
  int rc;
  if ((rc = launch_fill_w_diag(ctx, m, zero_above))) return rc;
  const int64_t NP = m.NP;
  for (int64_t b = NB; b < NP; b *= 2) {
    const int64_t full = NP / (2 * b);               // pairs with a full-size second block
    const int64_t rag = NP - full * 2 * b;           // leftover rows; a ragged pair exists if rag > b
    for (int part = 0; part < 2; ++part) {
      int64_t npairs, b2, r0;
      if (part == 0) { npairs = full; b2 = b; r0 = 0; }
      else { npairs = (rag > b) ? 1 : 0; b2 = rag - b; r0 = full * 2 * b; }
      if (npairs == 0) continue;
      GemmArgs t{};   // T = L21 * W11
      t.m = (int)b2; t.n = (int)b; t.k = (int)b; t.alpha = 1.0; t.beta = 0.0;
      t.A = m.L + (r0 + b) * NP + r0; t.lda = NP; t.strideA = 2 * b * NP + 2 * b;
      t.B = m.W + r0 * NP + r0; t.ldb = NP; t.strideB = 2 * b * NP + 2 * b; t.b_lower = 1;
      t.C = m.tmp; t.ldc = b; t.strideC = b * b; t.batch = (int)npairs;
      if ((rc = launch_gemm(ctx, t))) return rc;
      GemmArgs w{};   // W21 = -W22 * T
      w.m = (int)b2; w.n = (int)b; w.k = (int)b2; w.alpha = -1.0; w.beta = 0.0;
      w.A = m.W + (r0 + b) * NP + (r0 + b); w.lda = NP; w.strideA = 2 * b * NP + 2 * b; w.a_lower = 1;
      w.B = m.tmp; w.ldb = b; w.strideB = b * b;
      w.C = m.W + (r0 + b) * NP + r0; w.ldc = NP; w.strideC = 2 * b * NP + 2 * b; w.batch = (int)npairs;
      if ((rc = launch_gemm(ctx, w))) return rc;
    }
  }
  return GPBO_OK;
}

static int copy_square(gpbo_ctx* ctx, const Model& m, const double* dev, double* out, int mode) {
  // mode 0: symmetric from lower; 1: lower with zero upper
  std::vector<double> h((size_t)m.NP * m.NP);
  GPBO_HIP(ctx, hipMemcpyAsync(h.data(), dev, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < m.N; ++i)
    for (int64_t j = 0; j < m.N; ++j) {
      double v;
      if (j <= i) v = h[i * m.NP + j];
      else v = mode == 0 ? h[j * m.NP + i] : 0.0;
      out[i * m.N + j] = v;
    }
  return GPBO_OK;
}

int build_acq_args(gpbo_ctx* ctx, const char* who, int acq, double acq_param, double y_max, int n_constraints,
                   const double* lb, const double* ub, int k_seeds, const void* best_idx, const void* best_val,
                   const void* seed_idx, const void* seed_val, AcqArgs* out) {
  if (!ctx) return GPBO_ERR_INVALID;
  const std::string w(who);
  const bool known = (acq >= GPBO_ACQ_UCB && acq <= GPBO_ACQ_LOG_EI) || acq == GPBO_ACQ_LOG_CEI || acq == GPBO_ACQ_LOG_FEAS;
  if (!known) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + ": unknown acquisition");
  if (n_constraints < 0 || n_constraints >= GPBO_MAX_MODELS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + ": bad n_constraints");
  if (acq == GPBO_ACQ_LOG_EI && n_constraints > 0)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + ": GPBO_ACQ_LOG_EI takes no constraints (n_constraints must be 0)");
  if (acq == GPBO_ACQ_LOG_FEAS && n_constraints == 0)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + ": GPBO_ACQ_LOG_FEAS needs at least one constraint (n_constraints must be >= 1)");
  if (acq == GPBO_ACQ_LOG_CEI && n_constraints == 0) acq = GPBO_ACQ_LOG_EI;      // the same key, made by the same instructions
  if (n_constraints > 0 && (!lb || !ub)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + ": lb/ub required");
  if (k_seeds < 0 || k_seeds > GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + ": k_seeds out of range [0, 64]");
  if (!best_idx || !best_val || (k_seeds > 0 && (!seed_idx || !seed_val))) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + ": NULL output");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  AcqArgs a{};
  a.acq = acq; a.param = acq_param; a.y_max = y_max; a.n_constraints = n_constraints;
  for (int j = 0; j <= n_constraints; ++j) {
    Model& m = ctx->models[j];
    if (!m.fitted || m.M_post != ctx->M || ctx->M < 1)
      GPBO_FAIL(ctx, GPBO_ERR_STATE, w + ": run gpbo_posterior for slots 0..n_constraints first");
    a.mu[j] = m.mu;
    a.sd[j] = m.sd;
  }
  for (int j = 0; j < n_constraints; ++j) { a.lb[j] = lb[j]; a.ub[j] = ub[j]; }
  *out = a;
  return GPBO_OK;
}

}  // namespace gpbo

using namespace gpbo;

extern "C" {

int gpbo_abi_version(void) { return GPBO_ABI_VERSION; }

const char* gpbo_last_error(const gpbo_ctx* ctx) {
  if (ctx) return ctx->err.c_str();
  std::lock_guard<std::mutex> lk(g_err_mu);
  static thread_local std::string copy;
  copy = g_err;
  return copy.c_str();
}

int gpbo_device_count(int* count) {
  if (!count) return GPBO_ERR_INVALID;
  *count = 0;
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    set_global_error(std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e));
    return GPBO_ERR_HIP;
  }
  return GPBO_OK;
}

int gpbo_create(int device, gpbo_ctx** out) {
  if (!out) return GPBO_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  int rc = gpbo_device_count(&n);
  if (rc) return rc;
  if (device < 0 || device >= n) GPBO_FAIL((gpbo_ctx*)nullptr, GPBO_ERR_INVALID, "gpbo_create: no such device");
  gpbo_ctx* ctx = new gpbo_ctx();
  ctx->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&ctx->info_dev, sizeof(int));
  if (e == hipSuccess) e = hipHostMalloc(&ctx->pinned, PIN_WINDOWS * PIN_WINDOW, hipHostMallocDefault);
  if (e == hipSuccess) ctx->pinned_aux = (char*)ctx->pinned + (PIN_WINDOWS - 1) * PIN_WINDOW;
  if (e == hipSuccess) {
    ctx->pinned_base = ctx->pinned;
    e = hipHostGetDevicePointer((void**)&ctx->pinned_base_dev, ctx->pinned_base, 0);
  }
  if (e == hipSuccess) e = hipHostMalloc(&ctx->small_pinned, SMALL_PIN_BYTES, hipHostMallocDefault);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->small_ev, hipEventDisableTiming);
  if (e == hipSuccess) {
    int* host_flag = (int*)((char*)ctx->pinned_aux + PIN_AUX_NEGVAR);
    *host_flag = 0;
    e = hipHostGetDevicePointer((void**)&ctx->negvar, host_flag, 0);
  }
  if (e != hipSuccess) {
    set_global_error(std::string("gpbo_create: ") + hipGetErrorString(e));
    delete ctx;
    return GPBO_ERR_HIP;
  }
  *out = ctx;
  return GPBO_OK;
}

int gpbo_destroy(gpbo_ctx* ctx) {
  if (!ctx) return GPBO_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  gpbo_comm_destroy(ctx);
  for (auto& m : ctx->models) free_model(m);
  for (auto& la : ctx->lookahead) {
    if (la.bulk) { (void)hipStreamSynchronize(la.bulk); (void)hipStreamDestroy(la.bulk); }
    for (auto ev : la.ev) (void)hipEventDestroy(ev);
  }
  ctx->lookahead.clear();
  for (auto& st : ctx->lml_stream) if (st) (void)hipStreamDestroy(st);
  for (auto& st : ctx->slot_stream) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  if (ctx->small_ev) (void)hipEventDestroy(ctx->small_ev);
  for (auto ev : ctx->kg_ev) if (ev) (void)hipEventDestroy(ev);
  for (StageClock* c : {&ctx->qnei_clock, &ctx->cnei_clock, &ctx->qnehvi_clock, &ctx->cnhvi_clock})
    for (auto ev : c->ev) if (ev) (void)hipEventDestroy(ev);
  for (auto ev : ctx->gen_ev) if (ev) (void)hipEventDestroy(ev);
  for (auto ev : ctx->ehvi_ev) if (ev) (void)hipEventDestroy(ev);
  if (ctx->small_pinned) (void)hipHostFree(ctx->small_pinned);
  if (ctx->polish_pinned) (void)hipHostFree(ctx->polish_pinned);
  if (ctx->fused_stage) (void)hipHostFree(ctx->fused_stage);
  if (ctx->info_slots) (void)hipFree(ctx->info_slots);
  for (auto& ln : ctx->lml_lane) if (ln.exec) (void)hipGraphExecDestroy(ln.exec);
  if (ctx->lml_slab) (void)hipFree(ctx->lml_slab);
  if (ctx->lml_X) (void)hipFree(ctx->lml_X);
  if (ctx->lml_y) (void)hipFree(ctx->lml_y);
  void* ptrs[] = {ctx->Xc, ctx->Xc_raw, ctx->Xcs, ctx->part, ctx->mu_part, ctx->ys, ctx->paths, ctx->cpaths, ctx->kg, ctx->ehvi, ctx->greedy, ctx->red, ctx->info_dev, ctx->comm_buf, ctx->kst, ctx->stage};
  if (ctx->comm_host) (void)hipHostFree(ctx->comm_host);
  if (ctx->mt_work) (void)hipFree(ctx->mt_work);
  if (ctx->mt_bits) (void)hipFree(ctx->mt_bits);
  if (ctx->mt_offset) (void)hipFree(ctx->mt_offset);
  if (ctx->mt_desc) (void)hipFree(ctx->mt_desc);

  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (ctx->pinned_base) (void)hipHostFree(ctx->pinned_base);
  for (auto& e : ctx->ev) {
    if (e.a) (void)hipEventDestroy(e.a);
    if (e.b) (void)hipEventDestroy(e.b);
  }
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return GPBO_OK;
}

int gpbo_synchronize(gpbo_ctx* ctx) {
  if (!ctx) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GPBO_OK;
}

int gpbo_device_info(gpbo_ctx* ctx, char* buf, int buflen) {
  if (!ctx || !buf || buflen < 64) return GPBO_ERR_INVALID;
  hipDeviceProp_t p;
  GPBO_HIP(ctx, hipGetDeviceProperties(&p, ctx->device));
  char pci[32] = "?";
  if (hipDeviceGetPCIBusId(pci, (int)sizeof(pci), ctx->device) != hipSuccess) { (void)hipGetLastError(); snprintf(pci, sizeof(pci), "?"); }
  snprintf(buf, buflen,
           "{\"name\": \"%s\", \"arch\": \"%s\", \"compute_units\": %d, \"clock_mhz\": %d, "
           "\"memory_clock_mhz\": %d, \"hbm_gib\": %.1f, \"l2_mib\": %.1f, \"lds_per_block_kib\": %.0f, "
           "\"device\": %d, \"pci_bus_id\": \"%s\", \"rank\": %d, \"world\": %d, \"rccl_nranks\": %d}",
           p.name, p.gcnArchName, p.multiProcessorCount, p.clockRate / 1000, p.memoryClockRate / 1000,
           (double)p.totalGlobalMem / (1024.0 * 1024.0 * 1024.0), (double)p.l2CacheSize / (1024.0 * 1024.0),
           (double)p.sharedMemPerBlock / 1024.0, ctx->device, pci, ctx->rank, ctx->world, comm_nranks(ctx));
  return GPBO_OK;
}

// The look-ahead side stream + events that belong to `main` (a stream about to be destroyed).
static void drop_lookahead(gpbo_ctx* ctx, hipStream_t main) {
  for (size_t i = 0; i < ctx->lookahead.size();) {
    if (ctx->lookahead[i].main != main) { ++i; continue; }
    for (auto ev : ctx->lookahead[i].ev) (void)hipEventDestroy(ev);
    if (ctx->lookahead[i].bulk) (void)hipStreamDestroy(ctx->lookahead[i].bulk);
    ctx->lookahead.erase(ctx->lookahead.begin() + (long)i);
  }
}

// Copies/fills that act on one buffer of EVERY lane (lane mode: the buffers of lane l sit l * lane_stride doubles
// behind lane 0's; host staging areas are arrays with `host_pitch` bytes per lane).
static hipError_t lane_memset(gpbo_ctx* ctx, void* p, size_t bytes) {
  if (ctx->lanes == 1) return hipMemsetAsync(p, 0, bytes, ctx->stream);
  return hipMemset2DAsync(p, (size_t)ctx->lane_stride * sizeof(double), 0, bytes, (size_t)ctx->lanes, ctx->stream);
}
static hipError_t lane_h2d(gpbo_ctx* ctx, void* dst, const void* src_host, size_t host_pitch, size_t bytes) {
  if (ctx->lanes == 1) return hipMemcpyAsync(dst, src_host, bytes, hipMemcpyHostToDevice, ctx->stream);
  return hipMemcpy2DAsync(dst, (size_t)ctx->lane_stride * sizeof(double), src_host, host_pitch, bytes, (size_t)ctx->lanes,
                          hipMemcpyHostToDevice, ctx->stream);
}
static hipError_t lane_d2h(gpbo_ctx* ctx, void* dst_host, size_t host_pitch, const void* src, size_t bytes) {
  if (ctx->lanes == 1) return hipMemcpyAsync(dst_host, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
  return hipMemcpy2DAsync(dst_host, host_pitch, src, (size_t)ctx->lane_stride * sizeof(double), bytes, (size_t)ctx->lanes,
                          hipMemcpyDeviceToHost, ctx->stream);
}

// The size tier of a model's fit (fit_plan.h; the two limits are read per call: debug-build switches)
static FitTier tier_of(const Model& m) { return fit_tier(m.NP, fused_max_np(), mid_max_np()); }

// X (N, d) | y (N) of a small host-side fit copied into the pinned staging window that belongs to ctx->pinned's window (0: the
// context's own stream, every such call ends with a stream synchronisation; 1 + slot: a gpbo_fit_begin in flight); the first
// kernel of the fit reads them there.
static int stage_small_inputs(gpbo_ctx* ctx, const Model& m, const double* X, const double* y_norm, const double** Xd, const double** yd) {
  if (!ctx->fused_stage) {
    GPBO_HIP(ctx, hipHostMalloc(&ctx->fused_stage, PIN_WINDOWS * FUSED_STAGE_BYTES, hipHostMallocDefault));
    GPBO_HIP(ctx, hipHostGetDevicePointer((void**)&ctx->fused_stage_dev, ctx->fused_stage, 0));
  }
  const size_t w = (size_t)((char*)ctx->pinned - (char*)ctx->pinned_base) / PIN_WINDOW;
  double* h = (double*)((char*)ctx->fused_stage + w * FUSED_STAGE_BYTES);
  memcpy(h, X, (size_t)m.N * m.d * sizeof(double));
  memcpy(h + (size_t)STAGE_NP_CAP * GPBO_MAX_DIM, y_norm, (size_t)m.N * sizeof(double));
  *Xd = (const double*)(ctx->fused_stage_dev + w * FUSED_STAGE_BYTES);
  *yd = *Xd + (size_t)STAGE_NP_CAP * GPBO_MAX_DIM;
  return GPBO_OK;
}

// Small problems (FitTier::Fused): the whole fit — or LML evaluation — as ONE launch of one workgroup per model
// (fused_small.hip; bitwise the multi-launch sequence below).  mode 0: fit incl. the packed W; 1 / 2: LML value / value + gradient.
// src 0: raw inputs (host arrays staged through pinned memory the kernel reads directly, or device arrays X_dev / y_dev) and the
// length scales of the pinned window; src 1: the model's resident Xs / yn / ls.  The pivot word and the LML scalars land in the
// pinned words *info_host / *out_host (valid after the stream has drained) without copy nodes.
static int enqueue_fused(gpbo_ctx* ctx, Model& m, const double* X, const double* y_norm, const double* X_dev, const double* y_dev,
                         double noise, int mode, int n_ls, int src, int** info_host, double** out_host, bool noise_grad = false) {
  int rc;
  m.noise = noise;
  const double *Xd = X_dev, *yd = y_dev;
  if (src == 0 && !X_dev && (rc = stage_small_inputs(ctx, m, X, y_norm, &Xd, &yd))) return rc;
  double* scal = m.tmp;
  if (mode != 0) {
    // (a lane group of gpbo_lml_batch has pointed red / cap_red at its slab's FB_SCAL region, which has exactly this size: nothing
    // grows there, and its LaunchScope puts back a pointer that is still the context's)
    char* p = (char*)ctx->red;
    int64_t cap = ctx->cap_red;
    if ((rc = ensure(ctx, &p, &cap, FIT_SCAL_DOUBLES * (int64_t)sizeof(double)))) return rc;
    ctx->red = p;
    ctx->cap_red = cap;
    scal = (double*)ctx->red;
  }
  const PinLane h = pin_lane(ctx->pinned);
  ev_begin(ctx, T_FIT);
  if (!ctx->no_timing) ctx->ev[T_KMAT].used = ctx->ev[T_CHOL].used = ctx->ev[T_TRTRI].used = false;   // one kernel: no phase events
  if ((rc = launch_fused_small(ctx, m, mode, src, n_ls, Xd, yd, pinned_dev(ctx, h.ls), scal, pinned_dev(ctx, h.info),
                               (int64_t)(PIN_INFO_PITCH / sizeof(int)), mode ? pinned_dev(ctx, h.out) : nullptr,
                               (int64_t)(PIN_OUT_PITCH / sizeof(double)), noise_grad)))
    return rc;
  if (mode == 0) m.wp_packed = true;
  else ev_end(ctx, T_FIT);
  *info_host = h.info;
  if (out_host) *out_host = h.out;
  return GPBO_OK;
}

// The strip path behind its inputs: K (quarter tiles) -> Cholesky -> W by column strips (+ the packed W of a fit) -> alpha; the
// pivot word reaches its pinned word from the last kernel.
static int factor_mid(gpbo_ctx* ctx, Model& m, double noise, bool pack, int** info_host) {
  int rc;
  m.noise = noise;
  if (!ctx->no_timing) ctx->ev[T_KMAT].used = ctx->ev[T_CHOL].used = ctx->ev[T_TRTRI].used = false;   // no phase events on this path
  if ((rc = launch_kmat_q(ctx, m, noise, m.L))) return rc;
  if ((rc = cholesky(ctx, m))) return rc;
  if ((rc = launch_w_strip(ctx, m, pack))) return rc;
  int* info_h = pin_lane(ctx->pinned).info;
  if ((rc = launch_alpha_strip(ctx, m, pinned_dev(ctx, info_h), (int64_t)(PIN_INFO_PITCH / sizeof(int))))) return rc;
  if (pack && m.Wp) m.wp_packed = true;
  *info_host = info_h;
  return GPBO_OK;
}

// K, L, W = L^-1 and alpha from the device-resident scaled inputs m.Xs / targets m.yn (m.N, m.NP, m.kernel set).
static int factor_resident(gpbo_ctx* ctx, Model& m, double noise, int** info_host, bool pack = true) {
  int rc;
  const FitTier tier = tier_of(m);
  if (tier == FitTier::Fused) return enqueue_fused(ctx, m, nullptr, nullptr, nullptr, nullptr, noise, 0, 0, 1, info_host, nullptr);   // (gpbo_fit_append's rebuild)
  m.noise = noise;
  GPBO_HIP(ctx, lane_memset(ctx, ctx->info_dev, sizeof(int)));
  if (tier == FitTier::Strip) return factor_mid(ctx, m, noise, pack, info_host);
  ev_begin(ctx, T_KMAT);
  if ((rc = launch_kmat(ctx, m, noise, m.L))) return rc;   // straight into the buffer the Cholesky factorises in place
  ev_end(ctx, T_KMAT);
  ev_begin(ctx, T_CHOL);
  if ((rc = cholesky(ctx, m))) return rc;
  ev_end(ctx, T_CHOL);
  int* info_h = pin_lane(ctx->pinned).info;   // one word per lane, PIN_INFO_PITCH apart
  GPBO_HIP(ctx, lane_d2h(ctx, info_h, PIN_INFO_PITCH, ctx->info_dev, sizeof(int)));
  // W and alpha are issued before the info check resolves (harmless on failure)
  ev_begin(ctx, T_TRTRI);
  if ((rc = trtri(ctx, m, pack))) return rc;      // (pack == false: an LML evaluation)
  ev_end(ctx, T_TRTRI);
  if ((rc = launch_trmv(ctx, m))) return rc;
  *info_host = info_h;
  return GPBO_OK;
}

// The shape / kernel / length-scale / noise checks of a fit or LML entry point (n_theta sets of n_ls length scales).
static int check_gp_args(gpbo_ctx* ctx, const char* who, int64_t N, int d, int kernel, const double* length_scales, int n_theta,
                         int n_ls, double noise) {
  const auto w = [who] { return std::string(who); };     // (built on a failure only)
  if (N < 1 || N > (1 << 16)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w() + ": N out of range [1, 65536]");
  if (d < 1 || d > GPBO_MAX_DIM) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, w() + ": d out of range [1, 64]");
  if (kernel != GPBO_KERNEL_RBF && kernel != GPBO_KERNEL_MATERN25 && kernel != GPBO_KERNEL_MATERN15 && kernel != GPBO_KERNEL_MATERN05)
    GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, w() + ": kernel must be RBF or Matern(nu=2.5, 1.5 or 0.5)");
  if (n_ls != 1 && n_ls != d) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w() + ": length_scale must have 1 or d entries");
  for (int64_t t = 0; t < (int64_t)n_theta * n_ls; ++t)
    if (!(length_scales[t] > 0.0) || !std::isfinite(length_scales[t]))
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, w() + ": length_scale must be positive and finite");
  if (!(noise >= 0.0)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w() + ": noise must be >= 0");
  return GPBO_OK;
}

// lane l's length scales into the window's staging words: one value for every dimension or one per dimension, 1 beyond d
static void stage_length_scales(void* window, int l, const double* length_scale, int n_ls, int d) {
  double* ls_h = pin_lane(window, l).ls;
  for (int t = 0; t < GPBO_MAX_DIM; ++t) ls_h[t] = (t < d) ? (n_ls == 1 ? length_scale[0] : length_scale[t]) : 1.0;
}

// Argument checks, buffers and descriptor of a fit; the scaled length scales go to the pinned staging words.  Nothing
// is enqueued (so this part stays outside a stream capture).
static int prepare_model(gpbo_ctx* ctx, Model& m, const char* who, bool have_inputs, int64_t N, int d, int kernel,
                         const double* length_scale, int n_ls, double noise, int precision) {
  int rc;
  if (!have_inputs || !length_scale) GPBO_FAIL(ctx, GPBO_ERR_INVALID, std::string(who) + ": NULL input");
  if ((rc = check_gp_args(ctx, who, N, d, kernel, length_scale, 1, n_ls, noise))) return rc;
  if (precision != GPBO_F64 && precision != GPBO_F32)
    GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, std::string(who) + ": precision must be GPBO_F64 or GPBO_F32");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));

  m.fitted = false;
  m.wp_packed = false;     // (set by the small fit paths at enqueue time; a failure before finish_enqueue must not leave it behind)
  m.wd_valid = false;      // W is about to change: the int8 digit planes of the old one must not be used
  m.wt_valid = false;      // (K no longer holds the transpose of this slot's W)
  m.M_post = -1;
  m.refreshable = false;   // (gpbo_posterior_refresh: a new fit has nothing to do with the resident posterior)
  m.amplitude = 1.0;       // a unit model until gpbo_fit_scaled says otherwise
  m.white = 0.0;
  const int64_t NP = round_up(N, NB);
  const int DP = pad_dim(d);
  if ((rc = alloc_model(ctx, m, NP, DP))) return rc;
  m.N = N; m.NP = NP; m.d = d; m.DP = DP; m.kernel = kernel; m.precision = precision;
  stage_length_scales(ctx->pinned, 0, length_scale, n_ls, d);
  return GPBO_OK;
}

// The fit enqueued on ctx->stream: inputs from the host (X, y_norm) or already on the device (X_dev raw (N, d), y_dev),
// then K, L, W, alpha.  With device inputs every operation is capturable into a hipGraph.
static int enqueue_factor(gpbo_ctx* ctx, Model& m, const double* X, const double* y_norm, const double* X_dev,
                          const double* y_dev, double noise, int** info_host, bool pack = true) {
  int rc;
  const int64_t N = m.N, NP = m.NP;
  const FitTier tier = tier_of(m);
  // scaled lanes read the resident inputs (lml_batch_run): a host-input sequence would run them at `noise` on unscaled targets
  if (ctx->lane_pair && !X_dev) GPBO_FAIL(ctx, GPBO_ERR_STATE, "scaled lanes need device-resident inputs");
  if (tier == FitTier::Fused) return enqueue_fused(ctx, m, X, y_norm, X_dev, y_dev, noise, 0, 0, 0, info_host, nullptr);
  if (tier == FitTier::Strip) {      // inputs straight from pinned host memory (or the resident device copies): no copy / fill nodes
    const double *Xd = X_dev, *yd = y_dev;
    if (!X_dev && (rc = stage_small_inputs(ctx, m, X, y_norm, &Xd, &yd))) return rc;
    ev_begin(ctx, T_FIT);
    if ((rc = launch_mid_inputs(ctx, m, Xd, yd, pinned_dev(ctx, pin_lane(ctx->pinned).ls)))) return rc;
    return factor_mid(ctx, m, noise, pack, info_host);
  }
  ev_begin(ctx, T_FIT);
  GPBO_HIP(ctx, lane_h2d(ctx, m.ls, pin_lane(ctx->pinned).ls, PIN_LS_PITCH, GPBO_MAX_DIM * sizeof(double)));
  GPBO_HIP(ctx, lane_memset(ctx, m.yn, (size_t)NP * sizeof(double)));
  if (X_dev) {
    if (ctx->lane_pair) {                    // scaled lanes: the window's [eta, ts] words to the lanes, targets y * ts_l
      GPBO_HIP(ctx, lane_h2d(ctx, ctx->lane_pair, pin_lane(ctx->pinned).pair, PIN_PAIR_PITCH, 2 * sizeof(double)));
      if ((rc = launch_lane_targets(ctx, y_dev, N, m.yn))) return rc;
    } else {
      for (int l = 0; l < ctx->lanes; ++l)     // every lane gets the same targets
        GPBO_HIP(ctx, hipMemcpyAsync(m.yn + (int64_t)l * ctx->lane_stride, y_dev, (size_t)N * sizeof(double),
                                     hipMemcpyDeviceToDevice, ctx->stream));
    }
    if ((rc = launch_prescale(ctx, X_dev, N, m.d, m.DP, m.ls, m.Xs, NP))) return rc;
  } else {
    GPBO_HIP(ctx, hipMemcpyAsync(m.tmp, X, (size_t)N * m.d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    GPBO_HIP(ctx, hipMemcpyAsync(m.yn, y_norm, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_prescale(ctx, m.tmp, N, m.d, m.DP, m.ls, m.Xs, NP))) return rc;
  }
  return factor_resident(ctx, m, noise, info_host, pack);
}

// Tail shared by the fit entry points: pack W for the posterior kernels (enqueue), then wait and resolve the pivot check.
static int finish_enqueue(gpbo_ctx* ctx, Model& m) {
  int rc;
  if (!m.wp_packed && (rc = launch_pack_w(ctx, m))) return rc;
  m.wp_packed = false;
  m.wd_valid = false;              // W changed: the int8 digit planes are re-packed by the next posterior that uses them
  if (m.precision == GPBO_F32) {   // fp32 posterior: W rounded to fp32 in f32-MFMA fragment order (fit itself is fp64)
    if ((rc = ensure(ctx, &m.Wp32, &m.cap_Wp32, m.NP * m.NP))) return rc;
    if ((rc = launch_pack_w32(ctx, m))) return rc;
  }
  ev_end(ctx, T_FIT);
  return GPBO_OK;
}

static int finish_wait(gpbo_ctx* ctx, Model& m, hipStream_t stream, int* info_h, int* info) {
  GPBO_HIP(ctx, hipStreamSynchronize(stream));
  if (*info_h != 0) {
    if (info) *info = *info_h;
    char b[160];
    snprintf(b, sizeof(b), "the kernel matrix is not positive definite: leading minor of order %d", *info_h);
    GPBO_FAIL(ctx, GPBO_ERR_NOT_PD, b);
  }
  m.fitted = true;
  return GPBO_OK;
}

static int finish_fit(gpbo_ctx* ctx, Model& m, int* info_h, int* info) {
  int rc = finish_enqueue(ctx, m);
  if (rc) return rc;
  return finish_wait(ctx, m, ctx->stream, info_h, info);
}

// a slot whose gpbo_fit_begin has not been waited for must not be refitted or read
static int no_pending_fit(gpbo_ctx* ctx, int slot, const char* who) {
  if (ctx->pending_info[slot])
    GPBO_FAIL(ctx, GPBO_ERR_STATE, std::string(who) + ": the slot has a pending gpbo_fit_begin (call gpbo_fit_wait first)");
  return GPBO_OK;
}

static int wait_all_pending_fits(gpbo_ctx* ctx) {
  for (int s = 0; s < GPBO_MAX_MODELS; ++s)
    if (ctx->pending_info[s]) {
      int rc = gpbo_fit_wait(ctx, s, nullptr);
      if (rc) return rc;
    }
  return GPBO_OK;
}

// gpbo_fit (amplitude 1, white 0) and gpbo_fit_scaled: the fit at `noise`; the slot keeps amplitude and white for its posteriors
static int fit_slot(gpbo_ctx* ctx, const char* who, int slot, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                    const double* length_scale, int n_ls, double noise, double amplitude, double white, int precision, int* info) {
  int* info_h = nullptr;
  int rc = check_slot(ctx, slot);
  if (rc) return rc;
  if ((rc = no_pending_fit(ctx, slot, who))) return rc;
  Model& m = ctx->models[slot];
  if ((rc = prepare_model(ctx, m, who, X && y_norm, N, d, kernel, length_scale, n_ls, noise, precision))) return rc;
  m.amplitude = amplitude;
  m.white = white;
  if ((rc = enqueue_factor(ctx, m, X, y_norm, nullptr, nullptr, noise, &info_h))) return rc;
  return finish_fit(ctx, m, info_h, info);
}

// amplitude > 0, white >= 0, alpha >= 0, all finite: what both scaled entry points require
static int check_scaled_args(gpbo_ctx* ctx, const char* who, double amplitude, double white, double alpha) {
  if (!scaled_args_ok(amplitude, white))
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, std::string(who) + ": amplitude must be > 0 and white >= 0, both finite");
  if (!(alpha >= 0.0) || !std::isfinite(alpha)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, std::string(who) + ": alpha must be >= 0 and finite");
  return GPBO_OK;
}

int gpbo_fit(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d,
             int kernel, const double* length_scale, int n_ls, double noise, int precision,
             int* info) {
  if (info) *info = 0;
  return fit_slot(ctx, "gpbo_fit", slot, X, y_norm, N, d, kernel, length_scale, n_ls, noise, 1.0, 0.0, precision, info);
}

int gpbo_fit_scaled(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                    const double* length_scale, int n_ls, double amplitude, double white, double alpha, int precision, int* info) {
  if (info) *info = 0;
  if (!ctx) return GPBO_ERR_INVALID;
  if (const int rc = check_scaled_args(ctx, "gpbo_fit_scaled", amplitude, white, alpha)) return rc;
  return fit_slot(ctx, "gpbo_fit_scaled", slot, X, y_norm, N, d, kernel, length_scale, n_ls, scaled_eta(amplitude, white, alpha),
                  amplitude, white, precision, info);
}

int gpbo_fit_begin(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                   const double* length_scale, int n_ls, double noise, int precision) {
  int rc = check_slot(ctx, slot);
  if (rc) return rc;
  if ((rc = no_pending_fit(ctx, slot, "gpbo_fit_begin"))) return rc;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->slot_stream[slot]) GPBO_HIP(ctx, hipStreamCreateWithFlags(&ctx->slot_stream[slot], hipStreamNonBlocking));
  if (!ctx->info_slots) GPBO_HIP(ctx, hipMalloc((void**)&ctx->info_slots, GPBO_MAX_MODELS * sizeof(int)));
  int* info_h = nullptr;
  {
    // the slot's own stream, pinned window and pivot word for the duration of the enqueue (as a gpbo_lml_batch group)
    LaunchScope scope(ctx);
    ctx->stream = ctx->slot_stream[slot];
    ctx->pinned = pin_window(ctx, 1 + slot);
    ctx->info_dev = ctx->info_slots + slot;
    ctx->no_timing = true;            // the timing events belong to the main stream's calls
    Model& m = ctx->models[slot];
    rc = prepare_model(ctx, m, "gpbo_fit_begin", X && y_norm, N, d, kernel, length_scale, n_ls, noise, precision);
    if (rc == GPBO_OK) rc = enqueue_factor(ctx, m, X, y_norm, nullptr, nullptr, noise, &info_h);
    if (rc == GPBO_OK) rc = finish_enqueue(ctx, m);
  }
  if (rc) {
    (void)hipStreamSynchronize(ctx->slot_stream[slot]);     // nothing of a half-enqueued fit may still be running
    return rc;
  }
  ctx->pending_info[slot] = info_h;
  return GPBO_OK;
}

int gpbo_fit_wait(gpbo_ctx* ctx, int slot, int* info) {
  if (info) *info = 0;
  int rc = check_slot(ctx, slot);
  if (rc) return rc;
  if (!ctx->pending_info[slot]) GPBO_FAIL(ctx, GPBO_ERR_STATE, "gpbo_fit_wait: the slot has no pending gpbo_fit_begin");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  int* info_h = ctx->pending_info[slot];
  ctx->pending_info[slot] = nullptr;
  return finish_wait(ctx, ctx->models[slot], ctx->slot_stream[slot], info_h, info);
}

int gpbo_fit_append(gpbo_ctx* ctx, int slot, const double* x_new, int64_t n_new, int d,
                    const double* y_norm, int64_t n_total, int* info) {
  if (info) *info = 0;
  int rc = check_slot(ctx, slot);
  if (rc) return rc;
  if ((rc = no_pending_fit(ctx, slot, "gpbo_fit_append"))) return rc;
  Model& m = ctx->models[slot];
  if (!m.fitted) GPBO_FAIL(ctx, GPBO_ERR_STATE, "gpbo_fit_append: slot has no fitted model (call gpbo_fit first)");
  if (n_new < 0 || !y_norm || (n_new > 0 && !x_new)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "gpbo_fit_append: NULL input or n_new < 0");
  if (d != m.d) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "gpbo_fit_append: d differs from the fitted model's");
  if (n_total != m.N + n_new) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "gpbo_fit_append: n_total must be N + n_new");
  if (n_total > (1 << 16)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "gpbo_fit_append: N out of range [1, 65536]");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  m.fitted = false;
  m.wp_packed = false;
  m.wt_valid = false;
  const int64_t N0 = m.N;
  const int64_t NP_new = round_up(n_total, NB);
  const bool rebuild = (NP_new != m.NP) || n_new > 16;
  // gpbo_posterior_refresh: the resident mu / sd stay the posterior of their N_post rows over the current candidates when they
  // were valid for them coming in (or already stale but refreshable) and this call takes the row path; M_post = -1 either way
  const bool resident = (m.M_post == ctx->M && ctx->M >= 1) || (m.refreshable && m.M_refresh == ctx->M);
  const bool refreshable = resident && !rebuild && n_total - m.N_post <= 16 && n_total >= m.N_post;
  m.M_post = -1;
  m.refreshable = false;
  ev_begin(ctx, T_FIT);
  if (NP_new > m.cap_NP) {
    // grow the slot (25% head-room so that a maximize() loop reallocates rarely); the scaled inputs survive
    double* keep = nullptr;
    GPBO_HIP(ctx, hipMalloc((void**)&keep, (size_t)N0 * m.DP * sizeof(double)));
    GPBO_HIP(ctx, hipMemcpyAsync(keep, m.Xs, (size_t)N0 * m.DP * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    double* ls_h = pin_lane(ctx->pinned).ls;
    GPBO_HIP(ctx, hipMemcpyAsync(ls_h, m.ls, GPBO_MAX_DIM * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int DP = m.DP;
    const Model old = m;   // alloc_model resets the descriptor along with the buffers
    if ((rc = alloc_model(ctx, m, round_up(NP_new + NP_new / 4, NB), DP))) { (void)hipFree(keep); return rc; }
    m.N = old.N; m.NP = old.NP; m.d = old.d; m.DP = old.DP; m.kernel = old.kernel; m.precision = old.precision;
    m.noise = old.noise; m.amplitude = old.amplitude; m.white = old.white;
    GPBO_HIP(ctx, hipMemcpyAsync(m.ls, ls_h, GPBO_MAX_DIM * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    GPBO_HIP(ctx, hipMemcpyAsync(m.Xs, keep, (size_t)N0 * DP * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    GPBO_HIP(ctx, hipFree(keep));
  }
  // new rows: scaled into Xs[N0 .. NP_new) (zero padded), staged through ctx->Xcs-independent scratch (m.tvec is
  // too small for d > 1, m.tmp is free between fits)
  if (n_new > 0)
    GPBO_HIP(ctx, hipMemcpyAsync(m.tmp, x_new, (size_t)n_new * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (NP_new > N0)
    if ((rc = launch_prescale(ctx, m.tmp, n_new, d, m.DP, m.ls, m.Xs + N0 * m.DP, NP_new - N0))) return rc;
  GPBO_HIP(ctx, hipMemsetAsync(m.yn, 0, (size_t)NP_new * sizeof(double), ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(m.yn, y_norm, (size_t)n_total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  int* info_h = nullptr;
  if (rebuild) {
    m.N = n_total;
    m.NP = NP_new;
    if ((rc = factor_resident(ctx, m, m.noise, &info_h))) return rc;
  } else {
    GPBO_HIP(ctx, hipMemsetAsync(ctx->info_dev, 0, sizeof(int), ctx->stream));
    for (int64_t j = N0; j < n_total; ++j)
      if ((rc = launch_append_row(ctx, m, j))) return rc;
    m.N = n_total;
    info_h = pin_lane(ctx->pinned).info;
    GPBO_HIP(ctx, hipMemcpyAsync(info_h, ctx->info_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = launch_trmv(ctx, m))) return rc;
  }
  if ((rc = finish_fit(ctx, m, info_h, info))) return rc;
  m.refreshable = refreshable;
  m.M_refresh = refreshable ? ctx->M : -1;
  return GPBO_OK;
}

// The part of a log-marginal-likelihood evaluation that follows the factorisation, enqueued on ctx->stream: the scalar
// terms, K^-1 = W^T W and the gradient reduction, and the copy of the results to the pinned words *out_host.
static int lml_tail(gpbo_ctx* ctx, Model& m, int n_ls, int eval_gradient, double** out_host, bool noise_grad) {
  int rc;
  // the kernels write the scalars into the pinned words themselves (PIN_OUT_PITCH bytes per lane): no copy node
  double* out_h = pin_lane(ctx->pinned).out;
  double* out_d = pinned_dev(ctx, out_h);
  const int64_t pitch = (int64_t)(PIN_OUT_PITCH / sizeof(double));
  if (!eval_gradient && (rc = launch_lml_terms(ctx, m, out_d, pitch))) return rc;
  if (eval_gradient) {
    if (kinv_in_grad_launch(tier_of(m))) {      // kinv_grad_kernel; the two LML terms in its final launch
      if ((rc = launch_lml_grad(ctx, m, n_ls, nullptr, m.tmp, out_d, pitch, true, noise_grad))) return rc;
    } else {                                    // the W^T W GEMM into the K buffer, then the trace reduction; partials go to m.tmp
      GemmArgs g{};
      g.m = (int)m.NP; g.n = (int)m.NP; g.k = (int)m.NP; g.alpha = 1.0; g.beta = 0.0;
      g.A = m.W; g.lda = m.NP; g.a_trans = 1;
      g.B = m.W; g.ldb = m.NP;
      g.C = m.K; g.ldc = m.NP; g.batch = 1; g.lower_only = 1; g.k_from_tile = 1;
      if ((rc = launch_gemm(ctx, g))) return rc;
      if ((rc = launch_lml_grad(ctx, m, n_ls, m.K, m.tmp, out_d, pitch, true, noise_grad))) return rc;     // ... and the two LML terms
    }
  }
  ev_end(ctx, T_FIT);
  *out_host = out_h;
  return GPBO_OK;
}

// One log-marginal-likelihood evaluation of the prepared model m (and, in lane mode, of ctx->lanes models) enqueued on ctx->stream,
// inputs from the host (X, y_norm) or resident on the device (X_dev, y_dev): the one fused launch, or factorisation + tail.  Results
// land in the pinned words *out_host (yT alpha, sum log L_ii, gradient...) and *info_host once the stream has drained.
// noise_grad (with eval_gradient): the gradient's noise component g_eta as word 2 + n_ls (gpbo_lml_scaled).
static int enqueue_lml(gpbo_ctx* ctx, Model& m, const double* X, const double* y_norm, const double* X_dev, const double* y_dev,
                       double noise, int n_ls, int eval_gradient, double** out_host, int** info_host, bool noise_grad = false) {
  noise_grad = noise_grad && eval_gradient;
  if (tier_of(m) == FitTier::Fused)
    return enqueue_fused(ctx, m, X, y_norm, X_dev, y_dev, noise, eval_gradient ? 2 : 1, n_ls, 0, info_host, out_host, noise_grad);
  int rc = enqueue_factor(ctx, m, X, y_norm, X_dev, y_dev, noise, info_host, false);
  if (rc) return rc;
  return lml_tail(ctx, m, n_ls, eval_gradient, out_host, noise_grad);
}

static void lml_finish(const double* out_h, const int* info_h, int64_t N, int n_ls, int eval_gradient, double* lml,
                       double* grad, int* info) {
  if (*info_h != 0) {  // sklearn returns -inf and a zero gradient when K is not PD (_gpr.py:588-589)
    if (info) *info = *info_h;
    *lml = -INFINITY;
    if (eval_gradient) for (int t = 0; t < n_ls; ++t) grad[t] = 0.0;
    return;
  }
  *lml = -0.5 * out_h[0] - out_h[1] - 0.5 * (double)N * 1.83787706640934548356;  // log(2 pi)
  if (eval_gradient) for (int t = 0; t < n_ls; ++t) grad[t] = out_h[2 + t];
}

int gpbo_lml(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d,
             int kernel, const double* length_scale, int n_ls, double noise, int eval_gradient,
             double* lml, double* grad, int* info) {
  if (info) *info = 0;
  if (!lml || (eval_gradient && !grad)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "gpbo_lml: NULL output");
  int rc = check_slot(ctx, slot);
  if (rc) return rc;
  if ((rc = no_pending_fit(ctx, slot, "gpbo_lml"))) return rc;
  int* info_h = nullptr;
  double* out_h = nullptr;
  // the slot is left "unfitted": its W is not packed for the posterior kernel
  Model& m = ctx->models[slot];
  if ((rc = prepare_model(ctx, m, "gpbo_lml", X && y_norm, N, d, kernel, length_scale, n_ls, noise, GPBO_F64))) return rc;
  if ((rc = enqueue_lml(ctx, m, X, y_norm, nullptr, nullptr, noise, n_ls, eval_gradient, &out_h, &info_h))) return rc;
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  lml_finish(out_h, info_h, N, n_ls, eval_gradient, lml, grad, info);
  return GPBO_OK;
}

int gpbo_lml_scaled(gpbo_ctx* ctx, int slot, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                    const double* length_scale, int n_ls, double amplitude, double white, double alpha, int eval_gradient,
                    double* lml, double* grad, int* info) {
  if (info) *info = 0;
  if (!ctx) return GPBO_ERR_INVALID;
  if (!lml || (eval_gradient && !grad)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "gpbo_lml_scaled: NULL output");
  int rc = check_slot(ctx, slot);
  if (rc) return rc;
  if ((rc = check_scaled_args(ctx, "gpbo_lml_scaled", amplitude, white, alpha))) return rc;
  if ((rc = no_pending_fit(ctx, slot, "gpbo_lml_scaled"))) return rc;
  const double eta = scaled_eta(amplitude, white, alpha);
  int* info_h = nullptr;
  double* out_h = nullptr;
  // the unit model's evaluation U of the targets y / sqrt(c) at noise eta; the slot is left unfitted (and a unit model), as by gpbo_lml
  Model& m = ctx->models[slot];
  if ((rc = prepare_model(ctx, m, "gpbo_lml_scaled", X && y_norm, N, d, kernel, length_scale, n_ls, eta, GPBO_F64))) return rc;
  const double ts = scaled_target_scale(amplitude);
  std::vector<double> ys((size_t)N);       // (alive until the stream has drained below)
  for (int64_t i = 0; i < N; ++i) ys[(size_t)i] = y_norm[i] * ts;
  if ((rc = enqueue_lml(ctx, m, X, ys.data(), nullptr, nullptr, eta, n_ls, eval_gradient, &out_h, &info_h, true))) return rc;
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (*info_h != 0) {      // as gpbo_lml: -inf and a zero gradient
    if (info) *info = *info_h;
    *lml = -INFINITY;
    if (eval_gradient) for (int t = 0; t < n_ls + 2; ++t) grad[t] = 0.0;
    return GPBO_OK;
  }
  double unit = 0.0;
  lml_finish(out_h, info_h, N, n_ls, 0, &unit, nullptr, nullptr);
  *lml = scaled_lml(unit, N, amplitude);
  if (eval_gradient) scaled_lml_gradient(amplitude, white, alpha, N, out_h[0], out_h + 2, n_ls, out_h[2 + n_ls], grad);
  return GPBO_OK;
}

}  // extern "C"

namespace gpbo {
// The raw inputs of a theta search, resident on the device for every later gpbo_lml_batch call with X == y_norm == NULL
// (shared with gpbo_group_lml_batch, which puts them on every device of the group before it hands out lanes).
int lml_upload_inputs(gpbo_ctx* ctx, const double* X, const double* y_norm, int64_t N, int d) {
  if (!ctx || !X || !y_norm || N < 1 || d < 1) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "lml inputs: bad arguments");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  ctx->lml_N = 0;
  // On the context's own (non-blocking) stream, never the legacy stream: a synchronous hipMemcpy on one thread while another
  // thread's context captures its evaluation graph invalidates that capture on this runtime ("would make the legacy stream
  // depend on a capturing blocking stream"; seen with the lanes of a device group, one thread per device).
  std::shared_lock<std::shared_mutex> not_while_capturing(g_capture_mu);
  if ((rc = ensure(ctx, &ctx->lml_X, &ctx->cap_lml_X, N * d))) return rc;
  if ((rc = ensure(ctx, &ctx->lml_y, &ctx->cap_lml_y, N))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(ctx->lml_X, X, (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(ctx->lml_y, y_norm, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->lml_N = N; ctx->lml_d = d;
  return GPBO_OK;
}
}  // namespace gpbo

namespace gpbo {
// One workgroup that spins for `ticks` of the 100 MHz wall clock: the probe of pick_lane_streams.
__global__ void spin_ticks_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) {}
}

// Do one-workgroup kernels on streams a and b run side by side?  (100 us each: ~120 us side by side, ~220 one behind the other.)
static bool streams_overlap(hipStream_t a, hipStream_t b) {
  double best = 1e30;
  for (int r = 0; r < 3; ++r) {
    (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
    const auto t0 = std::chrono::steady_clock::now();
    spin_ticks_kernel<<<1, 64, 0, a>>>(10000);
    spin_ticks_kernel<<<1, 64, 0, b>>>(10000);
    (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
    best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  return best < 170.0;
}

// The streams of the lane groups of gpbo_lml_batch (n_groups > 1 from NP = 2048 on) must sit on DIFFERENT hardware queues, or the
// groups run one behind the other: the runtime deals its (four) queues to streams by load at creation time, and streams created at
// different moments of a process's life do collide — seen in round 6: the third group's stream, created when the first six-lane round
// of a search at N = 4096 came by, shared a queue with the first: 12.1 ms for the round against 10.0 with the streams created back
// to back (scripts/probes/stream_queues.hip: of eight streams created in a row the pairs (0,7), (1,6), (2,5), (3,4) serialise).
// So the streams are PICKED: a candidate is kept when a 100 us one-workgroup kernel on it runs side by side with one on every
// stream already chosen; rejected candidates are held until the picking is over (so that the next one lands elsewhere).  Once per
// context and group count, ~1 ms; the first four groups only (there are four queues).
static int pick_lane_streams(gpbo_ctx* ctx, int n_groups) {
  if (!ctx->lml_stream[0]) GPBO_HIP(ctx, hipStreamCreateWithFlags(&ctx->lml_stream[0], hipStreamNonBlocking));
  if (ctx->lane_streams_picked < 1) ctx->lane_streams_picked = 1;
  if (n_groups <= ctx->lane_streams_picked) return GPBO_OK;
  std::shared_lock<std::shared_mutex> not_while_capturing(g_capture_mu);
  std::vector<hipStream_t> rejected;
  for (int g = ctx->lane_streams_picked; g < n_groups; ++g) {
    if (ctx->lml_stream[g]) continue;
    hipStream_t cand = nullptr;
    for (int attempt = 0; attempt < 8; ++attempt) {
      GPBO_HIP(ctx, hipStreamCreateWithFlags(&cand, hipStreamNonBlocking));
      if (g >= 4) break;
      spin_ticks_kernel<<<1, 64, 0, cand>>>(100);          // (the first launch on a stream sets its queue up)
      bool ok = true;
      for (int c = 0; c < g && ok; ++c) ok = streams_overlap(ctx->lml_stream[c], cand);
      if (ok || attempt == 7) break;
      rejected.push_back(cand);
      cand = nullptr;
    }
    ctx->lml_stream[g] = cand;
  }
  for (auto st : rejected) (void)hipStreamDestroy(st);
  (void)hipGetLastError();
  ctx->lane_streams_picked = n_groups;
  return GPBO_OK;
}

// The graph pool of gpbo_lml_batch (ctx->lml_lane).  An evaluation is ~60 short launches: the second time the same problem shape
// comes by, the group's sequence is captured into a hipGraph and from then on replayed with one launch.

// The pool's entry for `key` — seen: the one that has run it — or the entry that takes it in: an unused one, else the least
// recently used, emptied (seen == false).  Either way it is now the most recently used.
static LmlLane& lml_lane_find(gpbo_ctx* ctx, const LmlKey& key) {
  LmlLane* found = nullptr;
  LmlLane* victim = &ctx->lml_lane[0];
  for (auto& e : ctx->lml_lane) {
    if (e.seen && e.key == key) {
      found = &e;
      break;
    }
    if ((!e.seen && victim->seen) || (e.seen == victim->seen && e.used < victim->used)) victim = &e;
  }
  LmlLane& e = found ? *found : *victim;
  if (!found) {
    if (e.exec) { (void)hipGraphExecDestroy(e.exec); e.exec = nullptr; }
    e.seen = false;
  }
  e.used = ++ctx->lml_lane_clock;
  return e;
}

static LmlKey lml_lane_key(const gpbo_ctx* ctx, const Model& m, int n_ls, int eval_gradient, int group, const double* gbase) {
  LmlKey k;
  k.N = m.N; k.d = m.d; k.kernel = m.kernel; k.n_ls = n_ls; k.eval_gradient = eval_gradient;
  k.scaled = ctx->lane_pair ? 1 : 0;
  k.noise = k.scaled ? 0.0 : m.noise;       // (a scaled group's noise is a word of its pinned window, not part of the sequence)
  k.lanes = ctx->lanes; k.group = group; k.X = ctx->lml_X; k.y = ctx->lml_y; k.K = gbase;
  return k;
}

// Group g's evaluation of m captured on ctx->stream (== ctx->lml_stream[g]) and instantiated into e.exec.  Failure leaves e.exec
// null, turns graphs off for the context and leaves ctx->stream a live stream for the direct launches that follow.
static void lml_lane_capture(gpbo_ctx* ctx, LmlLane& e, int g, Model& m, int n_ls, int eval_gradient) {
  hipGraph_t graph = nullptr;
  double* oh = nullptr; int* ih = nullptr;
  bool instantiated = false;
  {
    // Captures of different contexts (the lanes of a device group run on one thread per device) are taken one at a
    // time, process-wide: concurrent captures were seen to invalidate each other on this runtime
    // (tests/test_gpu_sharded.py, three virtual ranks).  A capture is ~1 ms of host work once per problem shape.
    std::unique_lock<std::shared_mutex> capture_lock(g_capture_mu);
    int crc = GPBO_ERR_HIP;
    hipError_t err = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
    if (err == hipSuccess) {
      crc = enqueue_lml(ctx, m, nullptr, nullptr, ctx->lml_X, ctx->lml_y, m.noise, n_ls, eval_gradient, &oh, &ih, ctx->lane_pair != nullptr);
      err = hipStreamEndCapture(ctx->stream, &graph);
    }
    instantiated = err == hipSuccess && crc == GPBO_OK && graph &&
                   hipGraphInstantiate(&e.exec, graph, nullptr, nullptr, 0) == hipSuccess && e.exec;
  }
  if (graph) (void)hipGraphDestroy(graph);
  if (instantiated) return;
  // capture is not available for this sequence on this runtime: direct launches from now on
  if (e.exec) { (void)hipGraphExecDestroy(e.exec); e.exec = nullptr; }
  (void)hipGetLastError();
  ctx->lml_graph_off = true;
  // an invalidated capture can outlive hipStreamEndCapture on this runtime: the direct launches need a live stream
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(ctx->stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    hipStream_t fresh = nullptr;
    if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) == hipSuccess) {
      drop_lookahead(ctx, ctx->lml_stream[g]);
      (void)hipStreamDestroy(ctx->lml_stream[g]);
      ctx->lml_stream[g] = fresh;
      ctx->stream = fresh;     // (the group's LaunchScope puts the context's own stream back)
    }
  }
}
}  // namespace gpbo

// What gpbo_lml_batch and gpbo_lml_batch_scaled share: the argument checks, the resident inputs, the lanes' evaluations enqueued
// group by group (direct launches or the group's graph) and the wait for the groups' streams.  The callers have checked n_theta's
// range and their pointers (lane_args_ok).  `pair` (scaled: [n_theta][eta, ts],
// else null): lane i runs at noise pair[2 i] on the targets y * pair[2 i + 1] and also reduces the gradient's noise component — the
// two words enter through the group's pinned window like the length scales, so a replayed graph reads each call's own.  On success
// lane i's words are in *groups_out's window 1 + i / per_group, lane i % per_group.
static int lml_batch_run(gpbo_ctx* ctx, const char* who, int n_theta, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                         const double* length_scales, int n_ls, double noise, const double* pair, int eval_gradient,
                         LaneGroups* groups_out) {
  const auto w = [who] { return std::string(who); };
  int rc = wait_all_pending_fits(ctx);   // their pinned windows are the ones the lane groups are about to use
  if (rc) return rc;
  const bool reuse_inputs = !X;     // X == y_norm == NULL: the inputs of the previous call are still on the device
  if (reuse_inputs && (ctx->lml_N != N || ctx->lml_d != d))
    GPBO_FAIL(ctx, GPBO_ERR_STATE, w() + ": no resident inputs of this shape (pass X and y_norm)");
  if ((rc = check_gp_args(ctx, who, N, d, kernel, length_scales, n_theta, n_ls, noise))) return rc;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));

  // One slab, one layout per lane: every kernel of the evaluation runs ONCE for all lanes (lane = a grid dimension,
  // lane l's buffers l * stride doubles behind lane 0's) — the command processor sees ~60 dispatches per batch, not
  // ~60 per theta.  Model slots and their fits are not touched.
  const int64_t NP = round_up(N, NB);
  const FitBuffers sizes = fit_buffers(NP, pad_dim(d));
  const LaneSlab slab = lane_slab(sizes);
  {
    std::shared_lock<std::shared_mutex> not_while_capturing(g_capture_mu);      // (hipMalloc / hipFree when the slab grows)
    if ((rc = ensure(ctx, &ctx->lml_slab, &ctx->cap_lml_slab, slab.stride * n_theta))) return rc;
  }
  if (!reuse_inputs && (rc = lml_upload_inputs(ctx, X, y_norm, N, d))) return rc;
  // the lanes in groups, a group's launch sequence once for its lanes on its own stream (fit_plan.h)
  const LaneGroups groups = lane_groups(NP, n_theta, env_override(dbg_env("GPBO_LML_PER_GROUP")));
  if ((rc = pick_lane_streams(ctx, groups.n_groups))) return rc;
  static const bool graphs_allowed = !(dbg_env("GPBO_LML_GRAPH") && dbg_env("GPBO_LML_GRAPH")[0] == '0');
  for (int g = 0; g < groups.n_groups && rc == GPBO_OK; ++g) {
    const int l0 = g * groups.per_group;
    double* gbase = ctx->lml_slab + (int64_t)l0 * slab.stride;
    LaunchScope scope(ctx);      // the group's stream, pinned window, scratch (exactly FIT_SCAL_DOUBLES: enqueue_fused) and lanes
    ctx->stream = ctx->lml_stream[g];
    ctx->pinned = pin_window(ctx, 1 + g);
    ctx->red = gbase + slab.off[FB_SCAL]; ctx->cap_red = sizes.size[FB_SCAL] * (int64_t)sizeof(double);
    ctx->info_dev = (int*)(gbase + slab.off[FB_INFO]);
    ctx->lanes = std::min(groups.per_group, n_theta - l0); ctx->lane_stride = slab.stride;
    ctx->lane_pair = pair ? gbase + slab.off[FB_INFO] + FIT_INFO_PAIR : nullptr;
    ctx->no_timing = true;
    ctx->no_lookahead = groups.n_groups > 1;
    Model m;     // a view of the group's first lane (not owning)
    m.N = N; m.NP = NP; m.d = d; m.DP = pad_dim(d); m.kernel = kernel; m.precision = GPBO_F64; m.noise = noise;
    const auto buf = model_buffers(m);
    for (int i = 0; i < FB_MODEL_COUNT; ++i) *buf[i] = gbase + slab.off[i];
    // theta enters through the pinned length-scale words ([lane][64]) that the sequence's first copy reads
    for (int l = 0; l < ctx->lanes; ++l) stage_length_scales(ctx->pinned, l, length_scales + (int64_t)(l0 + l) * n_ls, n_ls, d);
    for (int l = 0; pair && l < ctx->lanes; ++l) {      // ... and so do a scaled lane's noise and target scale
      double* ph = pin_lane(ctx->pinned, l).pair;
      ph[0] = pair[2 * (l0 + l)]; ph[1] = pair[2 * (l0 + l) + 1];
    }
    const LmlKey key = lml_lane_key(ctx, m, n_ls, eval_gradient, g, gbase);
    LmlLane& e = lml_lane_find(ctx, key);
    const bool graph = e.seen && graph_eligible(tier_of(m));      // from the second sighting on
    if (!graph && e.exec) { (void)hipGraphExecDestroy(e.exec); e.exec = nullptr; }
    if (graph && !e.exec && graphs_allowed && !ctx->lml_graph_off) lml_lane_capture(ctx, e, g, m, n_ls, eval_gradient);
    if (graph && e.exec) {
      GPBO_HIP(ctx, hipGraphLaunch(e.exec, ctx->stream));
      continue;
    }
    double* oh = nullptr; int* ih = nullptr;
    rc = enqueue_lml(ctx, m, nullptr, nullptr, ctx->lml_X, ctx->lml_y, noise, n_ls, eval_gradient, &oh, &ih, pair != nullptr);
    e.key = key;
    e.seen = (rc == GPBO_OK);
  }
  for (int g = 0; g < groups.n_groups; ++g) {
    hipError_t err = hipStreamSynchronize(ctx->lml_stream[g]);
    if (err != hipSuccess && rc == GPBO_OK) GPBO_HIP(ctx, err);
  }
  *groups_out = groups;
  return rc;
}

// 1 ... GPBO_LML_BATCH_MAX lanes, outputs and length scales given, X and y_norm both given or both NULL
static int lane_args_ok(gpbo_ctx* ctx, const char* who, int n_theta, const double* X, const double* y_norm, const double* length_scales,
                        int eval_gradient, const double* lml, const double* grad) {
  if (n_theta < 1 || n_theta > GPBO_LML_BATCH_MAX) GPBO_FAIL(ctx, GPBO_ERR_INVALID, std::string(who) + ": n_theta out of range [1, 8]");
  if (!lml || !length_scales || (eval_gradient && !grad) || (!X) != (!y_norm))
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, std::string(who) + ": NULL argument");
  return GPBO_OK;
}

// lane i's words of a finished batch
static PinLane batch_lane(const gpbo_ctx* ctx, const LaneGroups& groups, int i) {
  const int g = i / groups.per_group;
  return pin_lane(pin_window(ctx, 1 + g), i - g * groups.per_group);
}

extern "C" {

int gpbo_lml_batch(gpbo_ctx* ctx, int n_theta, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                   const double* length_scales, int n_ls, double noise, int eval_gradient, double* lml, double* grad,
                   int* info) {
  if (!ctx) return GPBO_ERR_INVALID;
  int rc = lane_args_ok(ctx, "gpbo_lml_batch", n_theta, X, y_norm, length_scales, eval_gradient, lml, grad);
  if (rc) return rc;
  LaneGroups groups{};
  if ((rc = lml_batch_run(ctx, "gpbo_lml_batch", n_theta, X, y_norm, N, d, kernel, length_scales, n_ls, noise, nullptr, eval_gradient,
                          &groups)))
    return rc;
  for (int i = 0; i < n_theta; ++i) {
    const PinLane h = batch_lane(ctx, groups, i);
    if (info) info[i] = 0;
    lml_finish(h.out, h.info, N, n_ls, eval_gradient, lml + i, eval_gradient ? grad + (size_t)i * n_ls : nullptr, info ? info + i : nullptr);
  }
  return GPBO_OK;
}

int gpbo_lml_batch_scaled(gpbo_ctx* ctx, int n_theta, const double* X, const double* y_norm, int64_t N, int d, int kernel,
                          const double* length_scales, int n_ls, const double* amplitudes, const double* whites, double alpha,
                          int eval_gradient, double* lml, double* grad, int* info) {
  if (!ctx) return GPBO_ERR_INVALID;
  int rc = lane_args_ok(ctx, "gpbo_lml_batch_scaled", n_theta, X, y_norm, length_scales, eval_gradient, lml, grad);
  if (rc) return rc;
  if (!amplitudes || !whites) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "gpbo_lml_batch_scaled: NULL argument");
  // lane i is the unit model's evaluation of the targets y / sqrt(c_i) at noise eta_i (scaled_kernel.h), as gpbo_lml_scaled runs it
  double pair[2 * GPBO_LML_BATCH_MAX];
  for (int i = 0; i < n_theta; ++i) {
    if ((rc = check_scaled_args(ctx, "gpbo_lml_batch_scaled", amplitudes[i], whites[i], alpha))) return rc;
    pair[2 * i] = scaled_eta(amplitudes[i], whites[i], alpha);
    pair[2 * i + 1] = scaled_target_scale(amplitudes[i]);
  }
  LaneGroups groups{};
  if ((rc = lml_batch_run(ctx, "gpbo_lml_batch_scaled", n_theta, X, y_norm, N, d, kernel, length_scales, n_ls, 0.0, pair, eval_gradient,
                          &groups)))
    return rc;
  const int n_g = n_ls + 2;
  for (int i = 0; i < n_theta; ++i) {
    const PinLane h = batch_lane(ctx, groups, i);
    if (info) info[i] = 0;
    double* g = eval_gradient ? grad + (size_t)i * n_g : nullptr;
    if (*h.info != 0) {      // as gpbo_lml_scaled: -inf and a zero gradient, this lane only
      if (info) info[i] = *h.info;
      lml[i] = -INFINITY;
      for (int t = 0; g && t < n_g; ++t) g[t] = 0.0;
      continue;
    }
    double unit = 0.0;
    lml_finish(h.out, h.info, N, n_ls, 0, &unit, nullptr, nullptr);
    lml[i] = scaled_lml(unit, N, amplitudes[i]);
    if (g) scaled_lml_gradient(amplitudes[i], whites[i], alpha, N, h.out[0], h.out + 2, n_ls, h.out[2 + n_ls], g);
  }
  return GPBO_OK;
}

static int need_fitted(gpbo_ctx* ctx, int slot) {
  int rc = check_slot(ctx, slot);
  if (rc) return rc;
  if (!ctx->models[slot].fitted) GPBO_FAIL(ctx, GPBO_ERR_STATE, "model slot has not been fitted");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return GPBO_OK;
}

int gpbo_get_K(gpbo_ctx* ctx, int slot, double* out) {
  int rc = need_fitted(ctx, slot);
  if (rc) return rc;
  // the fit assembles K directly into the buffer it factorises; the parity accessor re-assembles it from the
  // device-resident scaled inputs (same kernel, same bits)
  Model& m = ctx->models[slot];
  m.wt_valid = false;
  if ((rc = tier_of(m) == FitTier::Strip ? launch_kmat_q(ctx, m, m.noise, m.K) : launch_kmat(ctx, m, m.noise, m.K))) return rc;   // the fit's own kernel
  if ((rc = copy_square(ctx, m, m.K, out, 0))) return rc;
  if (m.amplitude != 1.0)      // a scaled slot holds the unit model K' = K / c
    for (int64_t i = 0; i < m.N * m.N; ++i) out[i] = scaled_K_entry(m.amplitude, out[i]);
  return GPBO_OK;
}
int gpbo_get_L(gpbo_ctx* ctx, int slot, double* out) {
  int rc = need_fitted(ctx, slot);
  if (rc) return rc;
  const Model& m = ctx->models[slot];
  if ((rc = copy_square(ctx, m, m.L, out, 1))) return rc;
  if (m.amplitude != 1.0)      // L_ = sqrt(c) L'
    for (int64_t i = 0; i < m.N * m.N; ++i) out[i] = scaled_L_entry(m.amplitude, out[i]);
  return GPBO_OK;
}
int gpbo_get_Linv(gpbo_ctx* ctx, int slot, double* out) {
  int rc = need_fitted(ctx, slot);
  if (rc) return rc;
  return copy_square(ctx, ctx->models[slot], ctx->models[slot].W, out, 1);
}
int gpbo_get_alpha(gpbo_ctx* ctx, int slot, double* out) {
  int rc = need_fitted(ctx, slot);
  if (rc) return rc;
  Model& m = ctx->models[slot];
  GPBO_HIP(ctx, hipMemcpyAsync(out, m.alpha, (size_t)m.N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (m.amplitude != 1.0)      // alpha_ = alpha' / c
    for (int64_t i = 0; i < m.N; ++i) out[i] = scaled_alpha_entry(m.amplitude, out[i]);
  return GPBO_OK;
}

int gpbo_set_candidates(gpbo_ctx* ctx, const double* Xc, int64_t M, int d) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!Xc || M < 1 || d < 1 || d > GPBO_MAX_DIM) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "set_candidates: bad arguments");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  ctx->raw_valid = false;
  if ((rc = ensure(ctx, &ctx->Xc, &ctx->cap_Xc, M * d))) return rc;
  const size_t bytes = (size_t)M * d * sizeof(double);
  if (bytes <= SMALL_PIN_IN) {
    // small batch: through the pinned block, no stream synchronisation (the block is reused only after its last copy)
    if (ctx->small_ev_pending) GPBO_HIP(ctx, hipEventSynchronize(ctx->small_ev));
    memcpy(ctx->small_pinned, Xc, bytes);
    GPBO_HIP(ctx, hipMemcpyAsync(ctx->Xc, ctx->small_pinned, bytes, hipMemcpyHostToDevice, ctx->stream));
    GPBO_HIP(ctx, hipEventRecord(ctx->small_ev, ctx->stream));
    ctx->small_ev_pending = true;
  } else {
    GPBO_HIP(ctx, hipMemcpyAsync(ctx->Xc, Xc, bytes, hipMemcpyHostToDevice, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  ctx->M = M;
  ctx->d_c = d;
  drop_posteriors(ctx);
  return GPBO_OK;
}

static int fetch_posterior(gpbo_ctx* ctx, Model& m, double* mu, double* sd);

int gpbo_posterior(gpbo_ctx* ctx, int slot, double y_mean, double y_std, double* mu, double* sd) {
  int rc = need_fitted(ctx, slot);
  if (rc) return rc;
  Model& m = ctx->models[slot];
  if (ctx->M < 1) GPBO_FAIL(ctx, GPBO_ERR_STATE, "posterior: no candidates resident (call gpbo_set_candidates)");
  if (ctx->d_c != m.d) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "posterior: candidate dimension differs from the fitted model");
  if ((rc = launch_posterior(ctx, m, ctx->M, y_mean, y_std))) return rc;
  return fetch_posterior(ctx, m, mu, sd);
}

// mu / sd of the resident candidates into the caller's arrays (either may be NULL: the results stay on the device)
static int fetch_posterior(gpbo_ctx* ctx, Model& m, double* mu, double* sd) {
  const size_t bytes = (size_t)ctx->M * sizeof(double);
  if ((mu || sd) && bytes <= SMALL_PIN_OUT) {      // small batch: results land in the pinned block, then in the caller's arrays
    double* hmu = (double*)((char*)ctx->small_pinned + SMALL_PIN_IN);
    double* hsd = (double*)((char*)ctx->small_pinned + SMALL_PIN_IN + SMALL_PIN_OUT);
    if (mu) GPBO_HIP(ctx, hipMemcpyAsync(hmu, m.mu, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (sd) GPBO_HIP(ctx, hipMemcpyAsync(hsd, m.sd, bytes, hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (mu) memcpy(mu, hmu, bytes);
    if (sd) memcpy(sd, hsd, bytes);
    return GPBO_OK;
  }
  if (mu) GPBO_HIP(ctx, hipMemcpyAsync(mu, m.mu, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (sd) GPBO_HIP(ctx, hipMemcpyAsync(sd, m.sd, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (mu || sd) GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GPBO_OK;
}

int gpbo_posterior_refresh(gpbo_ctx* ctx, int slot, double y_mean, double y_std, double* mu, double* sd, int* route) {
  if (route) *route = 0;
  int rc = need_fitted(ctx, slot);
  if (rc) return rc;
  Model& m = ctx->models[slot];
  // route 1: the resident mu / sd are the posterior of the slot's first N_post rows over the CURRENT candidates, and only row
  // appends have touched the slot since (the flag's keepers: gpbo_fit_append, prepare_model, drop_posteriors / drop_refreshable)
  const bool incremental = m.refreshable && m.M_refresh == ctx->M && ctx->M >= 1 && ctx->d_c == m.d && m.mu && m.sd &&
                           ctx->M <= m.cap_M && m.N >= m.N_post && m.N - m.N_post <= 16 && std::isfinite(m.ystd_post) &&
                           m.ystd_post != 0.0;
  if (!incremental) return gpbo_posterior(ctx, slot, y_mean, y_std, mu, sd);
  m.refreshable = false;
  if ((rc = launch_posterior_refresh(ctx, m, ctx->M, y_mean, y_std))) return rc;
  m.M_post = ctx->M;
  m.N_post = m.N;
  m.ystd_post = y_std;
  if (route) *route = 1;
  return fetch_posterior(ctx, m, mu, sd);
}

// The refusals gpbo_sample_paths (n_starts = 1) and gpbo_ascend_paths share, in their order; `missing`: what to say of a NULL
// argument, or null.  Hands back the slot's model.
static int check_path_args(gpbo_ctx* ctx, const char* who, int slot, double y_mean, double y_std, int n_paths, int n_features,
                           int n_starts, const char* missing, const Model** m) {
  int rc = check_slot(ctx, slot);
  if (rc) return rc;
  const std::string w = std::string(who) + ": ";
  if (n_paths < 1 || n_paths > GPBO_MAX_PATHS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_paths out of range [1, 16]");
  if (n_features < 1 || n_features > GPBO_MAX_PATH_FEATURES) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_features out of range [1, 4096]");
  if (n_starts < 1 || n_starts > GPBO_MAX_PATH_STARTS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_starts out of range [1, 8]");
  if (missing) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + missing);
  if (!std::isfinite(y_std) || !(y_std > 0.0) || !std::isfinite(y_mean))
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "y_std must be finite and positive, y_mean finite");
  if ((rc = no_pending_fit(ctx, slot, who))) return rc;
  if ((rc = need_fitted(ctx, slot))) return rc;
  *m = &ctx->models[slot];
  return GPBO_OK;
}

// The draws over the resident candidates (their negated values stay in ctx->ys) and the k best of each: best_idx / best_val the draws'
// maximisers, top_idx the rows' picks (null with k = 1: gpbo_sample_paths; else gpbo_ascend_paths' starts, and *ws has room for its runs)
static int draw_over_candidates(gpbo_ctx* ctx, const char* who, const Model& m, double y_mean, double y_std, int n_paths,
                                int n_features, const double* omega, const double* phase, const double* weights, const double* eps,
                                int k, int64_t index_offset, int64_t* best_idx, double* best_val, int64_t* top_idx,
                                PathWorkspace* ws) {
  int rc;
  const std::string w = std::string(who) + ": ";
  if (ctx->M < 1)
    GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "no candidates resident (call gpbo_set_candidates" + (top_idx ? ", or pass starts)" : ")"));
  if (ctx->d_c != m.d) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "the resident candidates' dimension differs from the fitted model's");
  const int64_t M = ctx->M;
  if (k > M) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_starts exceeds the number of resident candidates");
  if ((rc = launch_sample_paths(ctx, m, M, y_mean, y_std, n_paths, n_features, omega, phase, weights, eps, top_idx ? n_paths * k : 0,
                                ws)))
    return rc;
  if ((rc = launch_topk_rows(ctx, ctx->ys, M, n_paths, M, k, index_offset, best_idx, best_val, top_idx))) return rc;
  for (int s = 0; s < n_paths; ++s) best_val[s] = -best_val[s];      // the key is -f
  return GPBO_OK;
}

int gpbo_sample_paths(gpbo_ctx* ctx, int slot, double y_mean, double y_std, int n_paths, int n_features, const double* omega,
                      const double* phase, const double* weights, const double* eps, int64_t index_offset, int64_t* best_idx,
                      double* best_val, double* values_out) {
  const Model* m;
  PathWorkspace ws{};
  const bool given = omega && phase && weights && eps && best_idx && best_val;
  int rc = check_path_args(ctx, "sample_paths", slot, y_mean, y_std, n_paths, n_features, 1, given ? nullptr : "NULL argument", &m);
  if (rc) return rc;
  if ((rc = draw_over_candidates(ctx, "sample_paths", *m, y_mean, y_std, n_paths, n_features, omega, phase, weights, eps, 1,
                                 index_offset, best_idx, best_val, nullptr, &ws)))
    return rc;
  if (values_out) {
    const int64_t n = (int64_t)n_paths * ctx->M;
    GPBO_HIP(ctx, hipMemcpyAsync(values_out, ctx->ys, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < n; ++i) values_out[i] = -values_out[i];
  }
  return GPBO_OK;
}

int gpbo_sample_paths_constrained(gpbo_ctx* ctx, int n_constraints, const double* y_mean, const double* y_std, const double* lb,
                                  const double* ub, int n_paths, int n_features, const double* omega, const double* phase,
                                  const double* weights, const double* eps, int64_t index_offset, int64_t* best_idx, double* best_val,
                                  double* best_viol, int* feasible_out, double* values_out, double* viol_out) {
  const char* who = "sample_paths_constrained";
  const std::string w = std::string(who) + ": ";
  if (!ctx) return GPBO_ERR_INVALID;
  const int C = n_constraints, S = n_paths, F = n_features;
  if (C < 1 || C > GPBO_MAX_MODELS - 1) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_constraints out of range [1, 7]");
  if (!y_mean || !y_std || !lb || !ub || !omega || !phase || !weights || !eps || !best_idx || !best_val || !best_viol || !feasible_out) {
    // the counts first, as check_path_args orders them
    if (S < 1 || S > GPBO_MAX_PATHS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_paths out of range [1, 16]");
    if (F < 1 || F > GPBO_MAX_PATH_FEATURES) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_features out of range [1, 4096]");
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "NULL argument");
  }
  int rc;
  const Model* ms[GPBO_MAX_MODELS];
  for (int j = 0; j <= C; ++j)
    if ((rc = check_path_args(ctx, who, j, y_mean[j], y_std[j], S, F, 1, nullptr, &ms[j]))) return rc;
  for (int j = 0; j < C; ++j)
    if (lb[j] != lb[j] || ub[j] != ub[j] || !(lb[j] < ub[j]))
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "the bounds must not be NaN, with lb < ub for every constraint");
  if (ctx->M < 1) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "no candidates resident (call gpbo_set_candidates)");
  for (int j = 0; j <= C; ++j)
    if (ctx->d_c != ms[j]->d) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "the resident candidates' dimension differs from a fitted model's");
  const int64_t M = ctx->M;
  const int d = ctx->d_c;
  const ConstrainedBlock b = constrained_block(S, M, ms[0]->DP, values_out != nullptr);
  if ((rc = ensure(ctx, &ctx->cpaths, &ctx->cap_cpaths, b.doubles))) return rc;
  double* viol = ctx->cpaths + b.viol;
  double* vals = values_out ? ctx->cpaths + b.vals : nullptr;
  // slot j's draws in the concatenated inputs
  const double* eps_of[GPBO_MAX_MODELS];
  {
    const double* e = eps;
    for (int j = 0; j <= C; ++j) { eps_of[j] = e; e += (int64_t)S * ms[j]->N; }
  }
  // the constraints in slot order (the violation's sum order), the objective last: its keys need the whole sum, and its path
  // weights stay in the workspace for the rows that fall back to the least violation
  PathWorkspace ws{};
  const size_t row_bytes = (size_t)S * (size_t)M * sizeof(double);
  for (int t = 1; t <= C + 1; ++t) {
    const int j = t <= C ? t : 0;
    const PathFold fold{path_epilogue(j), j ? lb[j - 1] : 0.0, j ? ub[j - 1] : 0.0, viol, vals};
    if ((rc = launch_sample_paths_fold(ctx, *ms[j], M, y_mean[j], y_std[j], S, F, omega + (int64_t)j * F * d, phase + (int64_t)j * F,
                                       weights + (int64_t)j * S * F, eps_of[j], fold, &ws)))
      return rc;
    if (values_out)      // stream order: the next slot's pass overwrites vals after this copy has read it
      GPBO_HIP(ctx, hipMemcpyAsync(values_out + (int64_t)j * S * M, vals, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (viol_out) GPBO_HIP(ctx, hipMemcpyAsync(viol_out, viol, row_bytes, hipMemcpyDeviceToHost, ctx->stream));
  // one selection over the keys; a row whose least key is +inf has no feasible candidate and takes its least violation
  if ((rc = launch_topk_rows(ctx, ctx->ys, M, S, M, 1, index_offset, best_idx, best_val, nullptr))) return rc;
  int64_t fallback_idx[GPBO_MAX_PATHS];
  int fallback_row[GPBO_MAX_PATHS], n_fallback = 0;
  for (int s = 0; s < S; ++s) {
    if (best_val[s] != best_val[s]) {
      best_viol[s] = best_val[s];
      feasible_out[s] = 0;
    } else if (best_val[s] == std::numeric_limits<double>::infinity()) {
      if ((rc = launch_topk_rows(ctx, viol + (int64_t)s * M, M, 1, M, 1, 0, best_idx + s, best_viol + s, nullptr))) return rc;
      fallback_idx[n_fallback] = best_idx[s];
      fallback_row[n_fallback++] = s;
      best_idx[s] += index_offset;
      feasible_out[s] = 0;
    } else {
      best_val[s] = -best_val[s];      // the key is -f
      best_viol[s] = 0.0;
      feasible_out[s] = 1;
    }
  }
  if (n_fallback) {
    double* f = ctx->cpaths + b.f;
    double host[GPBO_MAX_PATHS * GPBO_MAX_PATHS];
    if ((rc = launch_paths_at(ctx, *ms[0], ws, y_mean[0], y_std[0], S, F, fallback_idx, n_fallback, ctx->cpaths + b.pts, f,
                              GPBO_MAX_PATHS)))
      return rc;
    GPBO_HIP(ctx, hipMemcpyAsync(host, f, (size_t)S * GPBO_MAX_PATHS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < n_fallback; ++r) best_val[fallback_row[r]] = host[fallback_row[r] * GPBO_MAX_PATHS + r];
  }
  return GPBO_OK;
}

int gpbo_ascend_paths(gpbo_ctx* ctx, int slot, double y_mean, double y_std, int n_paths, int n_features, const double* omega,
                      const double* phase, const double* weights, const double* eps, int n_starts, const double* starts,
                      const double* box_lo, const double* box_hi, int max_iter, int64_t index_offset, int64_t* best_idx,
                      double* best_val, double* x_out, double* f_out, double* g_out, int* status_out, int* n_eval_out,
                      int64_t* start_idx_out) {
  const Model* m;
  const char* missing = nullptr;
  if (!omega || !phase || !weights || !eps || !box_lo || !box_hi || !x_out || !f_out || !status_out || !start_idx_out)
    missing = "NULL argument";
  else if (!starts && (!best_idx || !best_val)) missing = "NULL argument (best_idx / best_val without starts)";
  int rc = check_path_args(ctx, "ascend_paths", slot, y_mean, y_std, n_paths, n_features, n_starts, missing, &m);
  if (rc) return rc;
  for (int t = 0; t < m->d; ++t)
    if (!std::isfinite(box_lo[t]) || !std::isfinite(box_hi[t]) || !(box_lo[t] < box_hi[t]))
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, "ascend_paths: the box must be finite with box_lo < box_hi in every coordinate");
  if (max_iter < 0) max_iter = PATH_DEFAULT_MAX_ITER;
  const int R = n_paths * n_starts;
  PathWorkspace ws{};
  std::vector<int64_t> top;
  if (!starts) {
    top.resize((size_t)R);
    if ((rc = draw_over_candidates(ctx, "ascend_paths", *m, y_mean, y_std, n_paths, n_features, omega, phase, weights, eps, n_starts,
                                   index_offset, best_idx, best_val, top.data(), &ws)))
      return rc;
    for (int r = 0; r < R; ++r) start_idx_out[r] = top[r] >= 0 ? top[r] + index_offset : -1;
  } else {
    if ((rc = launch_path_weights(ctx, *m, n_paths, n_features, omega, phase, weights, eps, R, &ws))) return rc;
    for (int r = 0; r < R; ++r) start_idx_out[r] = -1;
  }
  return launch_path_ascent(ctx, *m, ws, n_paths, n_starts, n_features, y_mean, y_std, starts, starts ? nullptr : top.data(), box_lo,
                            box_hi, max_iter, x_out, f_out, g_out, status_out, n_eval_out);
}

int gpbo_predict(gpbo_ctx* ctx, int slot, const double* Xc, int64_t M, int d, double y_mean,
                 double y_std, double* mu, double* sd) {
  int rc = gpbo_set_candidates(ctx, Xc, M, d);
  if (rc) return rc;
  return gpbo_posterior(ctx, slot, y_mean, y_std, mu, sd);
}

int gpbo_take_negative_variance_flag(gpbo_ctx* ctx, int* seen) {
  if (!ctx || !seen) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "gpbo_take_negative_variance_flag: null argument");
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the finalize kernels of every enqueued posterior have written it
  int* flag = (int*)((char*)ctx->pinned_aux + PIN_AUX_NEGVAR);
  *seen = *flag;
  *flag = 0;
  return GPBO_OK;
}

int gpbo_predict_cov(gpbo_ctx* ctx, int slot, const double* Xc, int64_t M, int d, double y_mean, double y_std,
                     double* mu, double* cov) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!cov) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "predict_cov: NULL output");
  if (M < 1 || M > 16384) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "predict_cov: M out of range [1, 16384]");
  int rc = gpbo_set_candidates(ctx, Xc, M, d);
  if (rc) return rc;
  if ((rc = need_fitted(ctx, slot))) return rc;
  Model& m = ctx->models[slot];
  if (d != m.d) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "predict_cov: candidate dimension differs from the fitted model");
  if (mu) {   // the mean through the usual posterior path (_gpr.py:443-447)
    if ((rc = launch_posterior(ctx, m, M, y_mean, y_std))) return rc;
    GPBO_HIP(ctx, hipMemcpyAsync(mu, m.mu, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  double* cov_dev = nullptr;
  int64_t ldc = 0;
  if ((rc = launch_posterior_cov(ctx, m, M, y_std, &cov_dev, &ldc))) return rc;
  GPBO_HIP(ctx, hipMemcpy2DAsync(cov, (size_t)M * sizeof(double), cov_dev, (size_t)ldc * sizeof(double), (size_t)M * sizeof(double),
                                 (size_t)M, hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GPBO_OK;
}

int gpbo_predict_grad(gpbo_ctx* ctx, int slot, const double* Xc, int64_t M, int d, double y_mean, double y_std,
                      double* mu, double* sd, double* dmu, double* dsd) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!mu || !sd || !dmu || !dsd) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "predict_grad: NULL output");
  if (M < 1 || M > 4 * GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "predict_grad: M out of range [1, 256]");
  int rc = gpbo_set_candidates(ctx, Xc, M, d);
  if (rc) return rc;
  if ((rc = need_fitted(ctx, slot))) return rc;
  Model& m = ctx->models[slot];
  if (d != m.d) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "predict_grad: candidate dimension differs from the fitted model");
  double *dmu_dev = nullptr, *dsd_dev = nullptr;
  if ((rc = launch_posterior_grad(ctx, m, M, y_mean, y_std, &dmu_dev, &dsd_dev))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(mu, m.mu, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(sd, m.sd, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(dmu, dmu_dev, (size_t)M * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipMemcpyAsync(dsd, dsd_dev, (size_t)M * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return GPBO_OK;
}

int gpbo_acq_argbest(gpbo_ctx* ctx, int acq, double acq_param, double y_max, int n_constraints,
                     const double* lb, const double* ub, int k_seeds, int64_t index_offset,
                     int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val,
                     double* ys_out) {
  AcqArgs a{};
  int rc = build_acq_args(ctx, "acq_argbest", acq, acq_param, y_max, n_constraints, lb, ub, k_seeds, best_idx, best_val,
                          seed_idx, seed_val, &a);
  if (rc) return rc;
  ev_begin(ctx, T_ACQ);
  rc = launch_acq_argbest(ctx, a, ctx->M, k_seeds, index_offset, best_idx, best_val, seed_idx, seed_val);
  ev_end(ctx, T_ACQ);
  if (rc) return rc;
  if (ys_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(ys_out, ctx->ys, (size_t)ctx->M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GPBO_OK;
}

int gpbo_mes_argbest(gpbo_ctx* ctx, int n_samples, const double* y_star, int k_seeds, int64_t index_offset, int64_t* best_idx,
                     double* best_val, int64_t* seed_idx, double* seed_val, double* ys_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (n_samples < 1 || n_samples > GPBO_MAX_MES_SAMPLES) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "mes_argbest: n_samples out of range [1, 64]");
  if (!y_star) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "mes_argbest: NULL y_star");
  for (int s = 0; s < n_samples; ++s)
    if (!std::isfinite(y_star[s])) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "mes_argbest: y_star must be finite");
  if (k_seeds < 0 || k_seeds > GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "mes_argbest: k_seeds out of range [0, 64]");
  if (!best_idx || !best_val || (k_seeds > 0 && (!seed_idx || !seed_val))) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "mes_argbest: NULL output");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  const Model& m = ctx->models[0];
  if (!m.fitted || m.M_post != ctx->M || ctx->M < 1) GPBO_FAIL(ctx, GPBO_ERR_STATE, "mes_argbest: run gpbo_posterior for slot 0 first");
  ev_begin(ctx, T_ACQ);
  int rc = launch_mes_values(ctx, m, ctx->M, n_samples, y_star);
  if (!rc) rc = launch_values_argbest(ctx, ctx->M, k_seeds, index_offset, best_idx, best_val, seed_idx, seed_val);
  ev_end(ctx, T_ACQ);
  if (rc) return rc;
  if (ys_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(ys_out, ctx->ys, (size_t)ctx->M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GPBO_OK;
}

int gpbo_kg_argbest(gpbo_ctx* ctx, const double* points, int n_points, int d, double y_mean, double y_std, int k_seeds,
                    int64_t index_offset, int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val, double* ys_out,
                    double* mu_points_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (n_points < 1 || n_points > GPBO_MAX_KG_POINTS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: n_points out of range [1, 64]");
  if (d < 1 || d > GPBO_MAX_DIM) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: d out of range");
  if (!points) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: NULL points");
  for (int64_t e = 0; e < (int64_t)n_points * d; ++e)
    if (!std::isfinite(points[e])) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: points must be finite");
  if (k_seeds < 0 || k_seeds > GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: k_seeds out of range [0, 64]");
  if (!best_idx || !best_val || (k_seeds > 0 && (!seed_idx || !seed_val))) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: NULL output");
  if (!std::isfinite(y_std) || !(y_std > 0.0) || !std::isfinite(y_mean))
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: y_std must be finite and positive, y_mean finite");
  int rc = no_pending_fit(ctx, 0, "kg_argbest");
  if (rc) return rc;
  if ((rc = need_fitted(ctx, 0))) return rc;
  const Model& m = ctx->models[0];
  if (d != m.d) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: the points' dimension differs from the fitted model's");
  if (ctx->M < 1 || m.M_post != ctx->M) GPBO_FAIL(ctx, GPBO_ERR_STATE, "kg_argbest: run gpbo_posterior for slot 0 first");
  if (y_std != m.ystd_post)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "kg_argbest: y_std is not the one the resident posterior was scaled with");
  ev_begin(ctx, T_ACQ);
  rc = launch_kg_values(ctx, m, ctx->M, points, n_points, y_mean, y_std, mu_points_out);
  if (!rc) rc = launch_values_argbest(ctx, ctx->M, k_seeds, index_offset, best_idx, best_val, seed_idx, seed_val);
  ev_end(ctx, T_ACQ);
  if (rc) return rc;
  if (ys_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(ys_out, ctx->ys, (size_t)ctx->M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GPBO_OK;
}

// The refusals gpbo_ehvi_argbest and gpmo_cehvi_argbest share, in the order the former has always had them; w: "<who>: ".
// ... of the arguments
static int check_ehvi_args(gpbo_ctx* ctx, const std::string& w, int nobj, const int* n_levels, const double* levels, int64_t n_cells,
                           const uint8_t* cell_lo, const uint8_t* cell_hi, int k_seeds, const void* best_idx, const void* best_val,
                           const void* seed_idx, const void* seed_val) {
  if (nobj < 2 || nobj > GPBO_MAX_EHVI_OBJECTIVES) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_objectives out of range [2, 3]");
  if (!n_levels || !levels || !cell_lo || !cell_hi) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "NULL levels or cells");
  for (int j = 0; j < nobj; ++j) {
    if (n_levels[j] < 2 || n_levels[j] > GPBO_MAX_EHVI_LEVELS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "a level count out of range [2, 130]");
    const double* row = levels + (size_t)j * GPBO_MAX_EHVI_LEVELS;
    for (int l = 0; l + 1 < n_levels[j]; ++l)
      if (!std::isfinite(row[l]) || !(row[l] < row[l + 1]))
        GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "levels must be finite and strictly increasing up to the last");
    if (!(row[n_levels[j] - 1] == INFINITY)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "the last level must be +inf");
  }
  if (n_cells < 1 || n_cells > GPBO_MAX_EHVI_CELLS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_cells out of range [1, 16641]");
  for (int64_t k = 0; k < n_cells; ++k)
    for (int j = 0; j < nobj; ++j)
      if ((int)cell_hi[k * nobj + j] >= n_levels[j] || cell_lo[k * nobj + j] >= cell_hi[k * nobj + j])
        GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "a cell needs lo < hi < the objective's level count");
  if (k_seeds < 0 || k_seeds > GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "k_seeds out of range [0, 64]");
  if (!best_idx || !best_val || (k_seeds > 0 && (!seed_idx || !seed_val))) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "NULL output");
  return GPBO_OK;
}
// ... of the state of slots 0 .. n_slots - 1 (what: "every objective's slot" / "every objective's and constraint's slot")
static int check_ehvi_slots(gpbo_ctx* ctx, const char* who, int n_slots, const char* what) {
  int rc;
  for (int j = 0; j < n_slots; ++j) {
    if ((rc = no_pending_fit(ctx, j, who))) return rc;
    if ((rc = need_fitted(ctx, j))) return rc;
  }
  const std::string w = std::string(who) + ": ";
  if (ctx->M < 1) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "no candidates");
  for (int j = 0; j < n_slots; ++j)
    if (ctx->models[j].M_post != ctx->M) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "run gpbo_posterior for " + what + " first");
  return GPBO_OK;
}
// ... and what follows the values in ctx->ys: the selection, the outputs, ys_out
static int ehvi_finish(gpbo_ctx* ctx, int rc, int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val, int64_t* seed_idx,
                       double* seed_val, double* ys_out) {
  if (!rc) rc = launch_values_argbest(ctx, ctx->M, k_seeds, index_offset, best_idx, best_val, seed_idx, seed_val);
  ev_end(ctx, T_ACQ);
  if (rc) return rc;
  if (ys_out) {
    GPBO_HIP(ctx, hipMemcpyAsync(ys_out, ctx->ys, (size_t)ctx->M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GPBO_OK;
}

int gpbo_ehvi_argbest(gpbo_ctx* ctx, int n_objectives, const int* n_levels, const double* levels, int64_t n_cells,
                      const uint8_t* cell_lo, const uint8_t* cell_hi, int k_seeds, int64_t index_offset, int64_t* best_idx,
                      double* best_val, int64_t* seed_idx, double* seed_val, double* ys_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  const int nobj = n_objectives;
  int rc = check_ehvi_args(ctx, "ehvi_argbest: ", nobj, n_levels, levels, n_cells, cell_lo, cell_hi, k_seeds, best_idx, best_val,
                           seed_idx, seed_val);
  if (rc) return rc;
  if ((rc = check_ehvi_slots(ctx, "ehvi_argbest", nobj, "every objective's slot"))) return rc;
  ev_begin(ctx, T_ACQ);
  rc = launch_ehvi_values(ctx, nobj, ctx->M, n_levels, levels, n_cells, cell_lo, cell_hi);
  return ehvi_finish(ctx, rc, k_seeds, index_offset, best_idx, best_val, seed_idx, seed_val, ys_out);
}

int gpmo_cehvi_argbest(gpbo_ctx* ctx, int n_objectives, const int* n_levels, const double* levels, int64_t n_cells,
                       const uint8_t* cell_lo, const uint8_t* cell_hi, int n_constraints, const double* lb, const double* ub,
                       int log_form, int k_seeds, int64_t index_offset, int64_t* best_idx, double* best_val, int64_t* seed_idx,
                       double* seed_val, double* ys_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  const int nobj = n_objectives, C = n_constraints;
  const std::string w = "cehvi_argbest: ";
  int rc = check_ehvi_args(ctx, w, nobj, n_levels, levels, n_cells, cell_lo, cell_hi, k_seeds, best_idx, best_val, seed_idx, seed_val);
  if (rc) return rc;
  if (C < 1 || C > GPBO_MAX_MODELS - nobj)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_constraints out of range [1, " + std::to_string(GPBO_MAX_MODELS - nobj) + "]");
  if (!lb || !ub) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "NULL lb or ub");
  for (int j = 0; j < C; ++j)
    if (lb[j] != lb[j] || ub[j] != ub[j] || !(lb[j] < ub[j]))
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "the bounds must not be NaN, with lb < ub for every constraint");
  if (log_form != 0 && log_form != 1) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "log_form must be 0 or 1");
  if ((rc = check_ehvi_slots(ctx, "cehvi_argbest", nobj + C, "every objective's and constraint's slot"))) return rc;
  ev_begin(ctx, T_ACQ);
  rc = launch_cehvi_values(ctx, nobj, ctx->M, n_levels, levels, n_cells, cell_lo, cell_hi, C, lb, ub, log_form);
  return ehvi_finish(ctx, rc, k_seeds, index_offset, best_idx, best_val, seed_idx, seed_val, ys_out);
}

// The refusals the greedy draw batches (gpbo_qnei_greedy, gpbo_qnhvi_greedy, gpbo_cnei_greedy) share, in three pieces that each
// entry point calls in its own order; w: "<who>: ".
// ... of the entry points over several slots: the counts (as check_path_args orders them), a NULL argument, then check_path_args
// per slot 0 .. n_slots - 1
static int check_greedy_slots(gpbo_ctx* ctx, const char* who, int n_groups, int n_paths, int n_features, bool given, int n_slots,
                              const double* y_mean, const double* y_std, const Model** ms) {
  const std::string w = std::string(who) + ": ";
  if (n_groups < 1 || n_groups > GPBO_MAX_QNEI_GROUPS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_groups out of range [1, 16]");
  if (n_paths < 1 || n_paths > GPBO_MAX_PATHS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_paths out of range [1, 16]");
  if (n_features < 1 || n_features > GPBO_MAX_PATH_FEATURES) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_features out of range [1, 4096]");
  if (!given) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "NULL argument");
  int rc;
  for (int j = 0; j < n_slots; ++j)
    if ((rc = check_path_args(ctx, who, j, y_mean[j], y_std[j], n_paths, n_features, 1, nullptr, &ms[j]))) return rc;
  return GPBO_OK;
}
// ... of the call's point set (noun: "pending" / "base"; at most `limit` points in the model's d dimensions, whose: "model's" /
// "models'")
static int check_greedy_points(gpbo_ctx* ctx, const std::string& w, const char* noun, const double* pts, int n, int limit, int d,
                               int model_d, const char* whose) {
  const std::string count = std::string("n_") + noun;
  if (n < 0 || n > limit) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + count + " out of range [0, " + std::to_string(limit) + "]");
  if (n > 0 && !pts) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "NULL " + noun + " with " + count + " > 0");
  if (d != model_d) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "d differs from the fitted " + whose);
  for (int64_t i = 0; i < (int64_t)n * d; ++i)
    if (!std::isfinite(pts[i])) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + noun + " must be finite");
  return GPBO_OK;
}
// ... of the resident candidates against every slot's model (whose: "the fitted model's" / "the fitted models'" / "a fitted model's")
static int check_greedy_candidates(gpbo_ctx* ctx, const std::string& w, int n_slots, const Model* const* ms, const char* whose, int q) {
  if (ctx->M < 1) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "no candidates resident (call gpbo_set_candidates)");
  for (int j = 0; j < n_slots; ++j)
    if (ctx->d_c != ms[j]->d) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "the resident candidates' dimension differs from " + whose);
  if (q > ctx->M) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "q exceeds the number of resident candidates");
  return GPBO_OK;
}

int gpbo_qnei_greedy(gpbo_ctx* ctx, int slot, double y_mean, double y_std, int n_groups, int n_paths, int n_features,
                     const double* omega, const double* phase, const double* weights, const double* eps, int noisy, double y_best,
                     const double* pending, int n_pending, int d, int q, int64_t index_offset, int64_t* pick_idx, double* pick_gain,
                     double* baseline_out, double* values_out, double* keys_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  const char* who = "qnei_greedy";
  const std::string w = std::string(who) + ": ";
  if (n_groups < 1 || n_groups > GPBO_MAX_QNEI_GROUPS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_groups out of range [1, 16]");
  const Model* m;      // (one slot: a NULL argument is check_path_args' `missing`, behind the slot and the counts)
  const bool given = omega && phase && weights && eps && pick_idx && pick_gain && baseline_out;
  int rc = check_path_args(ctx, who, slot, y_mean, y_std, n_paths, n_features, 1, given ? nullptr : "NULL argument", &m);
  if (rc) return rc;
  if (!noisy && !std::isfinite(y_best)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "y_best must be finite when noisy == 0");
  if ((rc = check_greedy_points(ctx, w, "pending", pending, n_pending, GPBO_MAX_QNEI_POINTS, d, m->d, "model's"))) return rc;
  if (q < 1 || q > GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "q out of range [1, 64]");
  if ((rc = check_greedy_candidates(ctx, w, 1, &m, "the fitted model's", q))) return rc;
  return launch_qnei_greedy(ctx, *m, ctx->M, y_mean, y_std, n_groups, n_paths, n_features, omega, phase, weights, eps, noisy, y_best,
                            pending, n_pending, q, index_offset, pick_idx, pick_gain, baseline_out, values_out, keys_out);
}

int gpbo_qnhvi_greedy(gpbo_ctx* ctx, const double* y_mean, const double* y_std, int n_groups, int n_paths, int n_features,
                       const double* omega, const double* phase, const double* weights, const double* eps, const double* ref,
                       const double* base, int n_base, int d, int q, int64_t index_offset, int64_t* pick_idx, double* pick_gain,
                       int* front_size_out, double* fronts_out, double* values_out, double* base_values_out, double* keys_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  const char* who = "qnehvi_greedy";
  const std::string w = std::string(who) + ": ";
  const bool given = y_mean && y_std && omega && phase && weights && eps && ref && pick_idx && pick_gain;
  const Model* ms[2];
  int rc = check_greedy_slots(ctx, who, n_groups, n_paths, n_features, given, 2, y_mean, y_std, ms);
  if (rc) return rc;
  if (!std::isfinite(ref[0]) || !std::isfinite(ref[1])) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "ref must be finite");
  if ((rc = check_greedy_points(ctx, w, "base", base, n_base, GPBO_MAX_QNEHVI_BASE, d, ms[0]->d, "models'"))) return rc;
  if (q < 1 || q > GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "q out of range [1, 64]");
  if (ms[1]->d != ms[0]->d) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "the two objectives' models differ in dimension");
  if ((rc = check_greedy_candidates(ctx, w, 2, ms, "the fitted models'", q))) return rc;
  return launch_qnehvi_greedy(ctx, ms, ctx->M, y_mean, y_std, n_groups, n_paths, n_features, omega, phase, weights, eps, ref, base,
                              n_base, q, index_offset, pick_idx, pick_gain, front_size_out, fronts_out, values_out, base_values_out,
                              keys_out);
}

int gpbo_cnei_greedy(gpbo_ctx* ctx, int n_constraints, const double* y_mean, const double* y_std, const double* lb, const double* ub,
                     int n_groups, int n_paths, int n_features, const double* omega, const double* phase, const double* weights,
                     const double* eps, double y_floor, const double* base, int n_base, int d, int q, int64_t index_offset,
                     int64_t* pick_idx, double* pick_gain, double* pick_feasible, double* baseline_out, double* values_out,
                     double* viol_out, double* base_values_out, double* keys_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  const char* who = "cnei_greedy";
  const std::string w = std::string(who) + ": ";
  const int C = n_constraints;
  if (C < 1 || C > GPBO_MAX_MODELS - 1) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_constraints out of range [1, 7]");
  const bool given = y_mean && y_std && lb && ub && omega && phase && weights && eps && pick_idx && pick_gain && pick_feasible && baseline_out;
  const Model* ms[GPBO_MAX_MODELS];
  int rc = check_greedy_slots(ctx, who, n_groups, n_paths, n_features, given, C + 1, y_mean, y_std, ms);
  if (rc) return rc;
  for (int j = 0; j < C; ++j)
    if (lb[j] != lb[j] || ub[j] != ub[j] || !(lb[j] < ub[j]))
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "the bounds must not be NaN, with lb < ub for every constraint");
  if (!std::isfinite(y_floor)) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "y_floor must be finite");
  if ((rc = check_greedy_points(ctx, w, "base", base, n_base, GPBO_MAX_CNEI_BASE, d, ms[0]->d, "models'"))) return rc;
  if (q < 1 || q > GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "q out of range [1, 64]");
  if ((rc = check_greedy_candidates(ctx, w, C + 1, ms, "a fitted model's", q))) return rc;
  return launch_cnei_greedy(ctx, C, ms, ctx->M, y_mean, y_std, lb, ub, n_groups, n_paths, n_features, omega, phase, weights, eps,
                            y_floor, base, n_base, q, index_offset, pick_idx, pick_gain, pick_feasible, baseline_out, values_out,
                            viol_out, base_values_out, keys_out);
}

int gpmo_cnhvi_greedy(gpbo_ctx* ctx, int n_constraints, const double* y_mean, const double* y_std, const double* lb, const double* ub,
                      int n_groups, int n_paths, int n_features, const double* omega, const double* phase, const double* weights,
                      const double* eps, const double* ref, const double* base, int n_base, int d, int q, int64_t index_offset,
                      int64_t* pick_idx, double* pick_gain, double* pick_feasible, int* front_size_out, double* fronts_out,
                      double* values_out, double* viol_out, double* base_values_out, double* keys_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  const char* who = "cnhvi_greedy";
  const std::string w = std::string(who) + ": ";
  const int C = n_constraints;
  if (C < 1 || C > GPBO_MAX_MODELS - 2) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "n_constraints out of range [1, 6]");
  const bool given = y_mean && y_std && lb && ub && omega && phase && weights && eps && ref && pick_idx && pick_gain && pick_feasible;
  const Model* ms[GPBO_MAX_MODELS];
  int rc = check_greedy_slots(ctx, who, n_groups, n_paths, n_features, given, C + 2, y_mean, y_std, ms);
  if (rc) return rc;
  for (int j = 0; j < C; ++j)
    if (lb[j] != lb[j] || ub[j] != ub[j] || !(lb[j] < ub[j]))
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "the bounds must not be NaN, with lb < ub for every constraint");
  if (!std::isfinite(ref[0]) || !std::isfinite(ref[1])) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "ref must be finite");
  if ((rc = check_greedy_points(ctx, w, "base", base, n_base, GPBO_MAX_QNEHVI_BASE, d, ms[0]->d, "models'"))) return rc;
  if (q < 1 || q > GPBO_MAX_SEEDS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, w + "q out of range [1, 64]");
  for (int j = 1; j < C + 2; ++j)
    if (ms[j]->d != ms[0]->d) GPBO_FAIL(ctx, GPBO_ERR_STATE, w + "the slots' models differ in dimension");
  if ((rc = check_greedy_candidates(ctx, w, C + 2, ms, "the fitted models'", q))) return rc;
  return launch_cnhvi_greedy(ctx, C, ms, ctx->M, y_mean, y_std, lb, ub, n_groups, n_paths, n_features, omega, phase, weights, eps, ref,
                             base, n_base, q, index_offset, pick_idx, pick_gain, pick_feasible, front_size_out, fronts_out,
                             values_out, viol_out, base_values_out, keys_out);
}

int gpbo_set_timing(gpbo_ctx* ctx, int on) {
  if (!ctx) return GPBO_ERR_INVALID;
  ctx->timing_off = !on;
  if (!on)
    for (int i = 0; i < T_COUNT; ++i) ctx->ev[i].used = false;     // gpbo_last_timings answers -1 from here on
  return GPBO_OK;
}

int gpbo_last_timings(gpbo_ctx* ctx, float* ms, int n) {
  if (!ctx || !ms) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < n; ++i) {
    ms[i] = -1.f;
    if (i < T_COUNT && ctx->ev[i].used) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ctx->ev[i].a, ctx->ev[i].b) == hipSuccess) ms[i] = t;
    }
  }
  return GPBO_OK;
}

#ifdef GPBO_DEBUG   // self-tests and micro-benchmarks: libgpbo_dbg.so only (include/gpbo.h, "debug build")
int gpbo_debug_cholesky(gpbo_ctx* ctx, const double* A, int64_t n, int variant, int iters, double* L_out, double* dinv_out,
                        long long* stamps_out, double* ms_out, int* info_out) {
  if (!ctx || !A || n < 64 || n % 64 || iters < 1 || variant != 3) return GPBO_ERR_INVALID;   // (variant 2, the round-2 schedule, is retired)
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  Model m;
  int rc = alloc_model(ctx, m, n, 4);
  if (rc) return rc;
  m.N = m.NP = n; m.d = 1; m.DP = 4;
  long long* stamps_dev = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  const size_t sq = (size_t)n * n * sizeof(double);
  auto done = [&](int code) {
    if (stamps_dev) (void)hipFree(stamps_dev);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    free_model(m);
    return code;
  };
  if (hipMalloc((void**)&stamps_dev, 16 * sizeof(long long)) != hipSuccess) return done(GPBO_ERR_HIP);
  (void)hipMemset(stamps_dev, 0, 16 * sizeof(long long));
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  m.wt_valid = false;
  if (hipMemcpy(m.K, A, sq, hipMemcpyHostToDevice) != hipSuccess) return done(GPBO_ERR_HIP);
  double best = 1e30;
  for (int it = 0; it < iters && !rc; ++it) {
    (void)hipMemcpyAsync(m.L, m.K, sq, hipMemcpyDeviceToDevice, ctx->stream);
    (void)hipMemsetAsync(ctx->info_dev, 0, sizeof(int), ctx->stream);
    (void)hipEventRecord(e0, ctx->stream);
    rc = cholesky(ctx, m, it == iters - 1 ? stamps_dev : nullptr);   // stamps: the last (warm) run
    (void)hipEventRecord(e1, ctx->stream);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return done(GPBO_ERR_HIP);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms < best) best = ms;
  }
  if (rc) return done(rc);
  if (ms_out) *ms_out = best;
  if (L_out && hipMemcpy(L_out, m.L, sq, hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  if (dinv_out && hipMemcpy(dinv_out, m.dinv, (size_t)(n / 64) * 4096 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return done(GPBO_ERR_HIP);
  if (stamps_out && hipMemcpy(stamps_out, stamps_dev, 16 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  if (info_out && hipMemcpy(info_out, ctx->info_dev, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  return done(GPBO_OK);
}

int gpbo_debug_gemm(gpbo_ctx* ctx, int m, int n, int k, double alpha, const double* A,
                    const double* B, int b_trans, double beta, double* C) {
  if (!ctx || !A || !B || !C) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  double *dA = nullptr, *dB = nullptr, *dC = nullptr;
  GPBO_HIP(ctx, hipMalloc((void**)&dA, (size_t)m * k * 8));
  GPBO_HIP(ctx, hipMalloc((void**)&dB, (size_t)n * k * 8));
  GPBO_HIP(ctx, hipMalloc((void**)&dC, (size_t)m * n * 8));
  GPBO_HIP(ctx, hipMemcpy(dA, A, (size_t)m * k * 8, hipMemcpyHostToDevice));
  GPBO_HIP(ctx, hipMemcpy(dB, B, (size_t)n * k * 8, hipMemcpyHostToDevice));
  GPBO_HIP(ctx, hipMemcpy(dC, C, (size_t)m * n * 8, hipMemcpyHostToDevice));
  GemmArgs g{};
  g.m = m; g.n = n; g.k = k; g.alpha = alpha; g.beta = beta;
  g.A = dA; g.lda = k; g.B = dB; g.ldb = b_trans ? k : n; g.b_trans = b_trans;
  g.C = dC; g.ldc = n; g.batch = 1;
  int rc = launch_gemm(ctx, g);
  if (!rc) {
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    GPBO_HIP(ctx, hipMemcpy(C, dC, (size_t)m * n * 8, hipMemcpyDeviceToHost));
  }
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
  return rc;
}

int gpbo_debug_gemm_bench(gpbo_ctx* ctx, int m, int n, int k, int b_trans, int a_trans, int lower_only, int iters,
                          double* out) {
  if (!ctx || !out || m < 64 || n < 64 || k < 16 || iters < 1 || (a_trans && b_trans)) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  double *dA = nullptr, *dB = nullptr, *dC = nullptr;
  const size_t na = (size_t)m * k, nb = (size_t)n * k, nc = (size_t)m * n;
  GPBO_HIP(ctx, hipMalloc((void**)&dA, na * 8));
  GPBO_HIP(ctx, hipMalloc((void**)&dB, nb * 8));
  GPBO_HIP(ctx, hipMalloc((void**)&dC, nc * 8));
  {
    // random (not zero) operands: the clock a kernel sustains depends on the data (MI355X_MICROARCH.md, DVFS)
    std::vector<double> h(std::max(na, nb));
    uint64_t sx = 0x9E3779B97F4A7C15ull;
    for (auto& v : h) { sx ^= sx << 13; sx ^= sx >> 7; sx ^= sx << 17; v = (double)(sx >> 11) * (1.0 / 9007199254740992.0) - 0.5; }
    GPBO_HIP(ctx, hipMemcpy(dA, h.data(), na * 8, hipMemcpyHostToDevice));
    GPBO_HIP(ctx, hipMemcpy(dB, h.data(), nb * 8, hipMemcpyHostToDevice));
    GPBO_HIP(ctx, hipMemset(dC, 0, nc * 8));
  }
  GemmArgs g{};
  g.m = m; g.n = n; g.k = k; g.alpha = 1.0; g.beta = 0.0;
  g.A = dA; g.lda = a_trans ? m : k; g.a_trans = a_trans;
  g.B = dB; g.ldb = b_trans ? k : n; g.b_trans = b_trans;
  g.C = dC; g.ldc = n; g.batch = 1; g.lower_only = lower_only;
  int rc = launch_gemm(ctx, g);    // warm-up
  hipEvent_t e0, e1;
  GPBO_HIP(ctx, hipEventCreate(&e0));
  GPBO_HIP(ctx, hipEventCreate(&e1));
  GPBO_HIP(ctx, hipEventRecord(e0, ctx->stream));
  for (int it = 0; it < iters && rc == GPBO_OK; ++it) rc = launch_gemm(ctx, g);
  GPBO_HIP(ctx, hipEventRecord(e1, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  GPBO_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
  const double flops = 2.0 * m * (double)n * k * (lower_only ? 0.5 : 1.0);
  out[0] = ms / iters;
  out[1] = flops / (ms / iters * 1e-3) / 1e12;
  return rc;
}

int gpbo_debug_select(gpbo_ctx* ctx, const double* ys, int64_t M, int k, int variant, int iters, int64_t* idx_out, double* val_out,
                      int64_t* first_nan_out, float* ms_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!ys || !idx_out || !val_out || M < 1 || k < 1 || k > GPBO_MAX_SEEDS || (variant != 1 && variant != 2) || iters < 0)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_select: bad arguments");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return debug_select(ctx, ys, M, k, variant, iters, idx_out, val_out, first_nan_out, ms_out);
}

int gpbo_debug_latency_probe(gpbo_ctx* ctx, long long* out, int n) {
  if (!ctx || !out || n < 1) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return run_latency_probe(ctx, out, n);
}

int gpbo_debug_kg_lines(gpbo_ctx* ctx, const double* a, const double* b, int64_t R, int n_lines, double* out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!a || !b || !out || R < 1 || R > (1 << 24) || n_lines < 1 || n_lines > GPBO_MAX_KG_POINTS + 1)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_kg_lines: bad arguments");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return debug_kg_lines(ctx, a, b, R, n_lines, out);
}

int gpbo_debug_kg_stage_ms(gpbo_ctx* ctx, float* ms) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!ms) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_kg_stage_ms: NULL output");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return debug_kg_stage_ms(ctx, ms);
}

// The stage clocks of the greedy draw batches (greedy.h: greedy_mark records them): ms[i] the kernel time between events i and
// i + 1 of `call`'s last run — qnei / cnei: the draws and baselines, the steps; qnehvi: the draws, the front build, the steps
static int greedy_stage_ms(gpbo_ctx* ctx, const StageClock& c, const std::string& who, const char* call, float* ms) {
  if (!ms) GPBO_FAIL(ctx, GPBO_ERR_INVALID, who + ": NULL output");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  if (!c.used) GPBO_FAIL(ctx, GPBO_ERR_STATE, who + ": no " + call + " call to report");
  GPBO_HIP(ctx, hipEventSynchronize(c.ev[c.n - 1]));
  for (int i = 0; i + 1 < c.n; ++i) GPBO_HIP(ctx, hipEventElapsedTime(&ms[i], c.ev[i], c.ev[i + 1]));
  return GPBO_OK;
}
int gpbo_debug_qnei_stage_ms(gpbo_ctx* ctx, float* ms) {
  if (!ctx) return GPBO_ERR_INVALID;
  return greedy_stage_ms(ctx, ctx->qnei_clock, "debug_qnei_stage_ms", "gpbo_qnei_greedy", ms);
}
int gpbo_debug_cnei_stage_ms(gpbo_ctx* ctx, float* ms) {
  if (!ctx) return GPBO_ERR_INVALID;
  return greedy_stage_ms(ctx, ctx->cnei_clock, "debug_cnei_stage_ms", "gpbo_cnei_greedy", ms);
}
int gpbo_debug_qnehvi_stage_ms(gpbo_ctx* ctx, float* ms) {
  if (!ctx) return GPBO_ERR_INVALID;
  return greedy_stage_ms(ctx, ctx->qnehvi_clock, "debug_qnehvi_stage_ms", "gpbo_qnhvi_greedy", ms);
}

int gpbo_debug_cnhvi_stage_ms(gpbo_ctx* ctx, float* ms) {
  if (!ctx) return GPBO_ERR_INVALID;
  return greedy_stage_ms(ctx, ctx->cnhvi_clock, "debug_cnhvi_stage_ms", "gpmo_cnhvi_greedy", ms);
}

int gpbo_debug_qnehvi_fronts(gpbo_ctx* ctx, int n_draws, int n, const double* base_values, const double* ref, int n_insert,
                             const double* insert_values, int* front_size_out, double* fronts_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (n_draws < 1 || n_draws > 4096 || n < 0 || n > GPBO_MAX_QNEHVI_BASE || n_insert < 0 || n_insert > 4096 || !ref ||
      !std::isfinite(ref[0]) || !std::isfinite(ref[1]) || (n > 0 && !base_values) || (n_insert > 0 && !insert_values) ||
      !front_size_out || !fronts_out)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_qnehvi_fronts: bad arguments");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return debug_qnehvi_fronts(ctx, n_draws, n, base_values, ref, n_insert, insert_values, front_size_out, fronts_out);
}

#endif  // GPBO_DEBUG

int gpbo_mfma_f64_peak(gpbo_ctx* ctx, int iters, double* tflops) {
  if (!ctx || !tflops || iters < 1) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return run_mfma_peak(ctx, iters, tflops);
}

int gpbo_mfma_f64_probe(gpbo_ctx* ctx, int iters, int waves_per_simd, int mode, double* out) {
  if (!ctx || !out || iters < 1 || waves_per_simd < 1 || waves_per_simd > 8) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return run_mfma_probe(ctx, iters, waves_per_simd, mode, out);
}

#ifdef GPBO_DEBUG
int gpbo_hybrid_probe(gpbo_ctx* ctx, int iters, int cfg, double* out) {
  if (!ctx || !out || iters < 1 || cfg < 0 || cfg > 4) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return run_hybrid_probe(ctx, iters, cfg, out);
}
#endif

int gpbo_hbm_copy_peak(gpbo_ctx* ctx, int64_t bytes, double* gbps) {
  if (!ctx || !gbps || bytes < (1 << 20)) return GPBO_ERR_INVALID;
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  return run_copy_peak(ctx, bytes, gbps);
}

}  // extern "C"
