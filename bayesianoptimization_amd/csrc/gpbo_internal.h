// Internal declarations shared by the HIP translation units of libgpbo (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <type_traits>

#include "gpbo.h"
#include "gpmo.h"
#include "fit_plan.h"         // the fit's size rule, its block size NB and a model's buffer sizes
#include "posterior_plan.h"   // the posterior's path rule and its row / candidate granules (POST_ROWS, POST_CANDS)
#include "search_plan.h"      // the one-launch searches' serve rule, LDS layouts and host / device blocks
#include "path_plan.h"        // the posterior function draws' workspace layout and dispatch rules
#include "cnei_plan.h"        // gpbo_cnei_greedy's workspace layout
#include "qnei_plan.h"        // gpbo_qnei_greedy's workspace layout and the score kernel's thread / candidate rule

namespace gpbo {

constexpr int POST_BK = 16;     // train points (k) per LDS stage of the fp64 kernels

enum TimingSlot {
  T_FIT = 0, T_POST_MAIN = 1, T_POST_FINAL = 2, T_ACQ = 3, T_KMAT = 4, T_CHOL = 5, T_TRTRI = 6, T_COUNT = 8
};

struct Model {
  bool fitted = false;
  bool wp_packed = false;  // the fused small-problem fit has already written Wp (finish_enqueue skips pack_w_kernel)
  bool wt_valid = false;   // K holds W^T for the slot's current fit (polish_fused.hip: the row walk of the local searches with W in memory)
  int64_t N = 0, NP = 0;   // observations, padded to a multiple of NB
  int d = 0, DP = 0;       // input dimension, padded to {4,8,16,32,64}
  int kernel = 0;
  int precision = 0;
  double noise = 0.0;      // value added to the diagonal of K at the last fit
  double amplitude = 1.0;  // c of a scaled model c * k + white * I (gpbo_fit_scaled): the fit itself is the unit-amplitude one at
  double white = 0.0;      // noise (white + alpha) / c; every place that turns |W k*|^2 into a variance applies c and white
  int64_t cap_NP = 0;      // allocated capacity (NP) of the square buffers
  int cap_DP = 0;
  double* ls = nullptr;    // [GPBO_MAX_DIM] length scale per dimension (device)
  double* Xs = nullptr;    // [NP][DP] train points / length_scale, zero padded
  double* K = nullptr;     // [NP][NP] kernel matrix + noise (lower triangle valid)
  double* L = nullptr;     // [NP][NP] Cholesky factor (lower triangle valid)
  double* W = nullptr;     // [NP][NP] L^-1 (upper triangle zero)
  double* Wp = nullptr;    // NP*NP doubles, MFMA-fragment packed W for the posterior kernel
  float* Wp32 = nullptr;   // NP*NP floats, W rounded to fp32 in v_mfma_f32_16x16x4_f32 fragment order (precision F32)
  int64_t cap_Wp32 = 0;
  uint4* Wd = nullptr;     // int8 digit planes of W, row-scaled (posterior_i8.hip), packed on first use after a fit
  int64_t cap_Wd = 0;
  double* wscale = nullptr; // [NP] power of two per row of W for the int8 GEMM's epilogue, then NP ints: the row exponents
  int64_t cap_wscale = 0;
  bool wd_valid = false;   // Wd / wscale hold the current fit's W
  double* dinv = nullptr;  // [NP/NB][NB][NB] inverses of the diagonal blocks of L
  double* tmp = nullptr;   // NP*NP/2 doubles workspace (trtri)
  double* yn = nullptr;    // [NP] normalised targets, zero padded
  double* tvec = nullptr;  // [NP] W*y
  double* alpha = nullptr; // [NP]
  // posterior outputs for the resident candidates
  double* mu = nullptr;
  double* sd = nullptr;
  int64_t cap_M = 0;
  int64_t M_post = -1;     // number of candidates mu/sd are valid for (-1: none)
  // gpbo_posterior_refresh: what the resident mu / sd reflect, recorded by the pass that wrote them ...
  int64_t N_post = 0;      // ... this many observations
  double ystd_post = 1.0;  // ... scaled with this y_std
  // ... and, once gpbo_fit_append's row path has made them stale (M_post = -1), whether they are still the posterior of the first
  // N_post rows over the context's current candidate set: "stale but refreshable".  Cleared by everything else that touches the
  // slot's fit (prepare_model, a rebuild inside append) and by every writer of the candidates (drop_refreshable below).
  bool refreshable = false;
  int64_t M_refresh = -1;  // the number of candidates they were valid for when they went stale
};

// gpbo_lml_batch, per lane group it has run: the problem shape and, from the second run on, the captured launch sequence.  A pool
// looked up by the whole key: the lanes of a call are dealt to groups by their number (gpbo_api.hip), and a theta search's rounds
// come with 6, 6, 5, 3, 2, 1, 1 ... live runs — every grouping it passes through keeps its graphs.
struct LmlKey {
  int64_t N = 0;
  int d = 0, kernel = 0, n_ls = 0, eval_gradient = 0, lanes = 0, group = 0;
  int scaled = 0;          // gpbo_lml_batch_scaled: noise and target scale per lane through the pinned window, `noise` stays 0
  double noise = 0.0;
  const void* X = nullptr; const void* y = nullptr; const void* K = nullptr;   // the resident inputs and the group's slab
  bool operator==(const LmlKey& o) const {
    return N == o.N && d == o.d && kernel == o.kernel && n_ls == o.n_ls && eval_gradient == o.eval_gradient && scaled == o.scaled &&
           noise == o.noise && lanes == o.lanes && group == o.group && X == o.X && y == o.y && K == o.K;
  }
};
struct LmlLane {
  LmlKey key;
  hipGraphExec_t exec = nullptr;
  bool seen = false;      // the key's sequence has been launched directly once: the next sighting captures it
  uint64_t used = 0;      // the pool's clock at its last use (the least recently used entry is the one replaced)
};
constexpr int LML_GRAPH_POOL = 24;

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  bool used = false;
};
// debug build: the n <= 4 events around the stages of an entry point's last call (greedy.h: greedy_mark; gpbo_api.hip: greedy_stage_ms); the
// product records nothing.  The fields exist in both builds: one layout.
struct StageClock {
  int n = 0;
  hipEvent_t ev[4] = {};
  bool used = false;
};

// Cholesky look-ahead (chol_kernels.hip): the bulk stream that carries the far part of a rank-512 trailing update while
// the next outer panel's chain runs on `main`, and the events the two streams hand each other.  One per main stream
// (the context's own, a slot's, an LML lane's), created on first use.
struct LookAhead {
  hipStream_t main = nullptr, bulk = nullptr;
  std::vector<hipEvent_t> ev;
};

}  // namespace gpbo

struct gpbo_ctx {
  int device = 0;
  int compute_units = 0;   // of the device, asked once (prepare_posterior_i8: the slab width that fills them)
  hipStream_t stream = nullptr;
  std::string err;
  gpbo::Model models[GPBO_MAX_MODELS];
  // gpbo_lml_batch: its stream (lml_stream[0]); the lanes' buffers live in lml_slab
  hipStream_t lml_stream[GPBO_LML_BATCH_MAX] = {};
  int lane_streams_picked = 0;   // how many of them were chosen to run side by side (pick_lane_streams, gpbo_api.hip)
  bool no_timing = false;   // batch lanes do not touch the timing events
  bool timing_off = false;  // gpbo_set_timing(ctx, 0): no event records at all (a record is a marker packet on the stream)
  bool no_lookahead = false;   // several lane streams in flight: the Cholesky look-ahead would only add streams to a full chip
  // gpbo_fit_begin / gpbo_fit_wait: a slot's fit enqueued on the slot's own stream, its staging words in pinned window
  // 1 + slot (the windows gpbo_lml_batch uses for its groups — it waits for pending fits first), its pivot word in info_slots
  hipStream_t slot_stream[GPBO_MAX_MODELS] = {};
  int* info_slots = nullptr;                       // device: GPBO_MAX_MODELS potrf info words
  int* pending_info[GPBO_MAX_MODELS] = {};         // host (pinned) word a pending fit's pivot check lands in; null = none
  // Lane mode (gpbo_lml_batch): every fit/LML launcher runs its kernel for `lanes` models at once; model l's buffers
  // sit l * lane_stride doubles behind the ones of the Model passed in (one slab, same layout per lane)
  int lanes = 1;
  int64_t lane_stride = 0;
  // gpbo_lml_batch_scaled: lane 0's [eta, target scale] on the device (lane l's l * lane_stride doubles behind), staged in the
  // pinned window's PIN_LANE_PAIR words; null: every lane runs at the launchers' `noise` with the targets as they are
  double* lane_pair = nullptr;
  double* lml_slab = nullptr; int64_t cap_lml_slab = 0;
  gpbo::LmlLane lml_lane[gpbo::LML_GRAPH_POOL];
  uint64_t lml_lane_clock = 0;
  double* lml_X = nullptr; int64_t cap_lml_X = 0;   // the batch's raw inputs, uploaded once per call
  double* lml_y = nullptr; int64_t cap_lml_y = 0;
  int64_t lml_N = 0; int lml_d = 0;                 // shape of the resident inputs (0: none)
  bool lml_graph_off = false;   // stream capture failed once: direct launches only
  // candidates
  double* Xc = nullptr;    // [M][d] raw
  int64_t cap_Xc = 0;      // capacity in doubles
  int64_t M = 0;
  int d_c = 0;
  double* Xc_raw = nullptr;   // [M][d] the candidates BEFORE gpbo_transform_candidates (what gpbo_get_candidate_rows returns then)
  int64_t cap_Xc_raw = 0;
  bool raw_valid = false;     // Xc holds kernel_transform(Xc_raw); cleared by everything that rewrites Xc
  double* stage = nullptr; // [d][M] stream-order image of device-generated candidates (mt19937.hip)
  int64_t cap_stage = 0;
  unsigned* mt_work = nullptr;   // MT19937 jump-ahead work area: returned state | 34-block stretch | sub-stream states
  int64_t cap_mt_work = 0;
  uint16_t* mt_bits = nullptr;   // jump polynomial table on the device (set-bit lists), its offsets, its stride and size
  int* mt_offset = nullptr;
  int64_t mt_table_stride = -1;
  int mt_table_count = 0;
  void* mt_desc = nullptr;       // sub-stream descriptors + polynomial indices of the current call (device)
  int64_t cap_mt_desc = 0;
  double* Xcs = nullptr;   // [Mp][DP] scaled/padded workspace
  int64_t cap_Xcs = 0;
  double* part = nullptr;  // [PostPlan::part_chunks][Mp] partial |W k*|^2 (the GEMV paths: their own scratch layout)
  int64_t cap_part = 0;
  double* mu_part = nullptr;  // [PostPlan::mu_chunks][Mp]: one partial mean per 256-train-point chunk (slab paths) or [Mp]
  int64_t cap_mu_part = 0;
  double* kst = nullptr;   // materialised k* slab [NP][slab width] (the posterior's slab paths)
  int64_t cap_kst = 0;
  double* ys = nullptr;    // [M] negated acquisition values ([n_paths][M] negated path values during gpbo_sample_paths)
  int64_t cap_ys = 0;
  double* kg = nullptr;    // gpbo_kg_argbest: the call's points, their solves and the candidate x point covariances (kg.hip)
  int64_t cap_kg = 0;
  double* ehvi = nullptr;  // gpbo_ehvi_argbest: the call's level rows, then one 8-byte word per cell (ehvi.hip)
  int64_t cap_ehvi = 0;
  double* greedy = nullptr;  // the workspace of whichever greedy draw batch runs — gpbo_qnei_greedy (qnei_plan.h), gpbo_cnei_greedy (cnei_plan.h), gpbo_qnhvi_greedy (qnehvi_plan.h): each call writes every part of its layout before it reads it, nothing is carried between calls
  int64_t cap_greedy = 0;
  hipEvent_t kg_ev[4] = {};   // debug build: around the three stages of the last gpbo_kg_argbest (the fields exist in both builds: one layout)
  bool kg_ev_used = false;
  hipEvent_t gen_ev[2] = {};  // debug build: around the kernel of the last gpbo_generate_candidates / _trust_region (generate_mark)
  bool gen_ev_used = false;
  gpbo::StageClock qnei_clock{3};   // before the draws, between the baselines and the greedy steps, behind the last step of the last gpbo_qnei_greedy
  gpbo::StageClock cnei_clock{3};   // the same three events of the last gpbo_cnei_greedy
  gpbo::StageClock qnehvi_clock{4}; // before the draws, behind them, behind the front build, behind the last step of the last gpbo_qnhvi_greedy
  gpbo::StageClock cnhvi_clock{4};  // the same four events of the last gpmo_cnhvi_greedy
  hipEvent_t ehvi_ev[2] = {}; // debug build: around the value kernel of the last gpbo_ehvi_argbest (ehvi.hip: ehvi_mark)
  bool ehvi_ev_used = false;
  double* paths = nullptr; // gpbo_sample_paths: features, weights and noise draws of the call | g(X) | W u | V (posterior_paths.hip)
  int64_t cap_paths = 0;
  double* cpaths = nullptr; // gpbo_sample_paths_constrained: viol | one slot's values | the fallback picks' points and values (path_plan.h)
  int64_t cap_cpaths = 0;
  void* red = nullptr;     // reduction scratch
  int64_t cap_red = 0;
  int* info_dev = nullptr; // potrf info word
  void* pinned = nullptr;  // pinned host staging: window 0 = fit/LML words (PIN_* below), windows 1..8 = gpbo_fit_begin slots / gpbo_lml_batch groups
  void* pinned_base = nullptr;      // the allocation `pinned` points into (never re-pointed) and the address the device sees it at:
  char* pinned_base_dev = nullptr;  // fused_small.hip reads length scales from it and writes pivot word / LML scalars into it
  void* fused_stage = nullptr;      // pinned: X / y of a small host-side fit per window (FUSED_STAGE_BYTES each), read by the fused kernel
  char* fused_stage_dev = nullptr;
  void* pinned_aux = nullptr;   // last window of the same allocation: selection / candidate staging (PIN_AUX_*); never re-pointed
  int* negvar = nullptr;        // device-visible address of the PIN_AUX_NEGVAR word
  // small batches (the host optimisers' rounds: tens to hundreds of points per call, hundreds of calls per suggest):
  // candidates and results cross PCIe through this pinned block instead of the caller's pageable arrays — the runtime
  // stages pageable copies through its own buffers and blocks on them, ~15-20 us per copy
  void* small_pinned = nullptr;          // SMALL_PIN_BYTES: [candidates in | mu out | sd out]
  void* polish_pinned = nullptr;         // gpbo_polish_seeds: [the round's points | per model [dmu | dsd | mu | sd] coming back]
  char* polish_pinned_dev = nullptr;     // ... as the device sees it: the round's kernels read / write it directly (no copy nodes)
  int64_t cap_polish_pinned = 0;
  hipEvent_t small_ev = nullptr;         // the last H2D out of small_pinned has completed
  bool small_ev_pending = false;
  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting: one bit per kernel family, per context (a
  // process-wide flag would leave every device but the first of a gpbo_group at the 64 KiB default)
  unsigned func_attrs = 0;
  std::vector<gpbo::LookAhead> lookahead;
  gpbo::EventPair ev[gpbo::T_COUNT];
  // RCCL
  void* comm = nullptr;          // ncclComm_t; exchanged atomically by whoever aborts it (comm.hip: abort_comm)
  bool comm_lost = false;        // the communicator was aborted after a collective failed or timed out
  bool debug_fail_next_acq = false;   // debug build: gpbo_debug_fail_next_acq armed (the field exists in both builds: one layout)
  int world = 1, rank = 0;
  void* comm_buf = nullptr;      // device: [send records | gathered records | 8-byte reduction word]
  int64_t cap_comm_buf = 0;
  void* comm_host = nullptr;     // pinned: gathered records / reduction word
  int64_t cap_comm_host = 0;
};

namespace gpbo {

constexpr size_t SMALL_PIN_IN = 128 * 1024, SMALL_PIN_OUT = 32 * 1024;   // bytes: candidates in; mu, sd out (each)
constexpr size_t SMALL_PIN_BYTES = SMALL_PIN_IN + 2 * SMALL_PIN_OUT;
constexpr unsigned ATTR_GEMM128 = 4u, ATTR_CHOL128 = 16u, ATTR_FUSED = 32u, ATTR_MID = 64u, ATTR_KINV_GRAD = 128u, ATTR_POLISH_FUSED = 256u, ATTR_GEMM_FAT = 512u, ATTR_EVOLVE = 2048u, ATTR_KG = 4096u, ATTR_EHVI = 8192u, ATTR_CEHVI = 16384u;
// pinned staging of a small host-side fit's X (N, d) | y (N), read by the first kernel directly (one window per PIN window)
constexpr int STAGE_NP_CAP = MID_NP_CAP;
static_assert(STAGE_NP_CAP >= FUSED_NP_CAP, "the staging window serves both small paths");
constexpr size_t FUSED_STAGE_BYTES = ((size_t)STAGE_NP_CAP * GPBO_MAX_DIM + STAGE_NP_CAP) * sizeof(double);

// ---- pinned host staging layout -------------------------------------------------------------------------------
// ONE allocation of PIN_WINDOWS windows of PIN_WINDOW bytes.  Window 0 (ctx->pinned) carries the words of a fit /
// LML evaluation; gpbo_fit_begin re-points ctx->pinned at window 1 + slot and gpbo_lml_batch at windows
// 1..GPBO_LML_BATCH_MAX for its groups (LaunchScope below); the LAST window (ctx->pinned_aux) belongs to the selection
// and candidate entry points, so that no two subsystems share a byte whatever stays in flight.
constexpr size_t PIN_WINDOW = 16384;
constexpr int PIN_WINDOWS = 2 + GPBO_LML_BATCH_MAX;
// every window but the last, one layout: per lane the length scales at +0, the potrf info words at PIN_LANE_INFO, the
// [eta, target scale] pair of a scaled lane at PIN_LANE_PAIR, the LML scalars (yT alpha, sum log L_ii, gradient[GPBO_MAX_DIM], the
// noise component) at PIN_LANE_OUT.  A single fit or evaluation is lane 0.
constexpr size_t PIN_LS_PITCH = GPBO_MAX_DIM * sizeof(double);
constexpr size_t PIN_INFO_PITCH = 8;
constexpr size_t PIN_OUT_PITCH = (3 + GPBO_MAX_DIM) * sizeof(double);
constexpr size_t PIN_PAIR_PITCH = 2 * sizeof(double);
constexpr size_t PIN_LANE_INFO = 4096, PIN_LANE_PAIR = 4096 + 256, PIN_LANE_OUT = 8192;
static_assert(GPBO_LML_BATCH_MAX * PIN_LS_PITCH <= PIN_LANE_INFO, "lane length scales overlap the lane info words");
static_assert(PIN_LANE_INFO + GPBO_LML_BATCH_MAX * PIN_INFO_PITCH <= PIN_LANE_PAIR, "lane info words overlap the lane noise / target-scale pairs");
static_assert(PIN_LANE_PAIR + GPBO_LML_BATCH_MAX * PIN_PAIR_PITCH <= PIN_LANE_OUT, "lane noise / target-scale pairs overlap the lane LML scalars");
static_assert(PIN_LANE_OUT + GPBO_LML_BATCH_MAX * PIN_OUT_PITCH <= PIN_WINDOW, "lane LML scalars leave the window");
// the address the device sees a word of the pinned window allocation at
template <typename T>
T* pinned_dev(const gpbo_ctx* ctx, T* host) { return (T*)(ctx->pinned_base_dev + ((const char*)host - (const char*)ctx->pinned_base)); }
inline void* pin_window(const gpbo_ctx* ctx, int w) { return (char*)ctx->pinned_base + PIN_WINDOW * (size_t)w; }
// lane l's words in a window (host addresses; the kernels take pinned_dev() of lane 0's and the pitches)
struct PinLane { double* ls; int* info; double* out; double* pair; };
inline PinLane pin_lane(void* window, int l = 0) {
  char* w = (char*)window;
  return {(double*)(w + (size_t)l * PIN_LS_PITCH), (int*)(w + PIN_LANE_INFO + (size_t)l * PIN_INFO_PITCH),
          (double*)(w + PIN_LANE_OUT + (size_t)l * PIN_OUT_PITCH), (double*)(w + PIN_LANE_PAIR + (size_t)l * PIN_PAIR_PITCH)};
}
// aux window
constexpr size_t PIN_AUX_SEL_OUT = 256;                              // SelState + picks[GPBO_MAX_SEEDS + 1] coming back
constexpr size_t PIN_AUX_SEL_OUT_BYTES = 32 + 16 * (GPBO_MAX_SEEDS + 1);
constexpr size_t PIN_AUX_CAND = 2048;                                // [lo | hi (or hi - lo)][GPBO_MAX_DIM] doubles | MT19937 key[624]
constexpr size_t PIN_AUX_CAND_BYTES = 2 * GPBO_MAX_DIM * sizeof(double) + 624 * sizeof(uint32_t);
static_assert(PIN_AUX_SEL_OUT + PIN_AUX_SEL_OUT_BYTES <= PIN_AUX_CAND, "selection results overlap the candidate staging");
constexpr size_t PIN_AUX_SEL_ROOM = PIN_AUX_CAND - PIN_AUX_SEL_OUT;      // all there is from the selection's window up to the candidate staging (gpbo_cnei_greedy's 24-byte pick records take it)
constexpr size_t PIN_AUX_NEGVAR = 8192;                              // int: a finalize kernel clipped a NEGATIVE variance (_gpr.py:479-485)
static_assert(PIN_AUX_CAND + PIN_AUX_CAND_BYTES <= PIN_AUX_NEGVAR, "candidate staging overlaps the clipped-variance flag");
static_assert(PIN_AUX_NEGVAR + sizeof(int) <= PIN_WINDOW, "clipped-variance flag leaves the window");

// The context's launch state — where the fit / LML launchers enqueue, stage and reduce, and for how many lanes — saved on
// construction and put back on destruction: gpbo_fit_begin and the lane groups of gpbo_lml_batch point it at a stream, a pinned
// window and scratch of their own for the duration of an enqueue, and every exit from that scope leaves the context as it was.
struct LaunchScope {
  gpbo_ctx* const ctx;
  const hipStream_t stream;
  void* const pinned;
  int* const info_dev;
  void* const red;
  const int64_t cap_red;
  const int lanes;
  const int64_t lane_stride;
  double* const lane_pair;
  const bool no_timing, no_lookahead;
  explicit LaunchScope(gpbo_ctx* c)
      : ctx(c), stream(c->stream), pinned(c->pinned), info_dev(c->info_dev), red(c->red), cap_red(c->cap_red), lanes(c->lanes),
        lane_stride(c->lane_stride), lane_pair(c->lane_pair), no_timing(c->no_timing), no_lookahead(c->no_lookahead) {}
  LaunchScope(const LaunchScope&) = delete;
  LaunchScope& operator=(const LaunchScope&) = delete;
  ~LaunchScope() {
    ctx->stream = stream; ctx->pinned = pinned; ctx->info_dev = info_dev; ctx->red = red; ctx->cap_red = cap_red;
    ctx->lanes = lanes; ctx->lane_stride = lane_stride; ctx->lane_pair = lane_pair; ctx->no_timing = no_timing; ctx->no_lookahead = no_lookahead;
  }
};

void set_global_error(const std::string& s);

// Environment policy.  The product library reads exactly four variables, none of which changes a result:
//   GPBO_KSTAR_GB (k* slab workspace budget), GPBO_COMM_TIMEOUT_S, GPBO_GROUP_TIMEOUT_S (deadlines of the multi-GPU
//   failure path) and GPBO_GROUP_HOST_MERGE (a device group merges its shards' records on the host instead of over RCCL).
// Everything else — A/B switches between kernel variants, dispatch thresholds, probes, fault injection — goes through
// dbg_env(), which is getenv() only in the -DGPBO_DEBUG build (libgpbo_dbg.so: the tests' and scripts' library) and a
// constant NULL in the product (tests/test_abi.py greps the sources for getenv against that allow-list).
#ifdef GPBO_DEBUG
inline const char* dbg_env(const char* name) { return getenv(name); }
#else
inline const char* dbg_env(const char*) { return nullptr; }
#endif
// a debug switch's number for the rules of fit_plan.h / search_plan.h: env_override(dbg_env("GPBO_..."))
inline int env_override(const char* e) { return e ? atoi(e) : NO_OVERRIDE; }
// the size cap of the one-launch searches (search_plan.h: search_max_np), local searches and evolution alike
inline int search_np_override() { return env_override(dbg_env("GPBO_POLISH_FUSED_MAX_NP")); }

#define GPBO_HIP(ctx, expr)                                                                  \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      char _b[512];                                                                          \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
               __FILE__, __LINE__);                                                          \
      if (ctx) (ctx)->err = _b;                                                              \
      gpbo::set_global_error(_b);                                                            \
      return GPBO_ERR_HIP;                                                                   \
    }                                                                                        \
  } while (0)

#define GPBO_FAIL(ctx, code, msg)                                                            \
  do {                                                                                       \
    if (ctx) (ctx)->err = (msg);                                                             \
    gpbo::set_global_error(msg);                                                             \
    return (code);                                                                           \
  } while (0)

// k(d2) for the posterior-side k* generation (device only).  Same formulas as sklearn (kernels.py:1722-1724,
// 1559-1560) with two cost cuts that stay within ~1 ulp: sqrt via v_rsq_f64 + Goldschmidt/Newton without the
// subnormal rescaling (d2 is a sum of squares of O(1) numbers; exact 0 handled), and K^2/3 as K^2 * (1/3).
// The fit-side kernel matrix (kmat_kernel) uses the same function, so K and k* share one arithmetic.
#ifdef __HIPCC__
// The refinement both roots share: from y = v_rsq_f64(x), g -> sqrt(x) and h -> 1 / (2 sqrt(x)) side by side (Goldschmidt), g closed
// by one Newton step.
__device__ __forceinline__ void gpbo_sqrt_refine(double x, double& g, double& h) {
  const double y = __builtin_amdgcn_rsq(x);
  g = x * y;
  h = 0.5 * y;
  double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  g = fma(fma(-g, g, x), h, g);
}
__device__ __forceinline__ double gpbo_sqrt_pos(double x) {
  double g, h;
  gpbo_sqrt_refine(x, g, h);
  return x > 0.0 ? g : x;   // 0 -> 0 (rsq(0) = inf would give NaN), NaN -> NaN
}
// exp(x) for x <= 0 (the only arguments a stationary kernel has): n = rint(x / ln 2), r = x - n ln 2 in two pieces (the high one
// has 32 significant bits, so n * ln2_hi and the first difference are exact for |n| < 2^11), exp(r) by the degree-13 Taylor
// polynomial (|r| <= 0.347: truncation 4e-18), result = ldexp(p, n) — v_ldexp_f64 rounds into the subnormals and to 0 by itself,
// x = 0 gives exactly 1, NaN stays NaN.  22 instructions against ~40 for the library's exp (which also serves x > 0, overflow
// and the errno-style cases); < 1 ulp (tests/test_gpu_parity.py::test_kernel_value_exp_against_numpy).  Round 4.
// Round 5: arguments below -800 are taken as -800 first (the result is an exact 0 from -745.2 on): for x = -inf the
// reduction was inf - inf = NaN (an RBF entry of points 1e160 apart: NumPy gives 0), and beyond |x| ~ 1e40 the reduced argument
// was garbage and the polynomial overflowed.  The comparison is false for NaN, which therefore still propagates.
__device__ __forceinline__ double gpbo_exp_nonpos(double x) {
  x = (x < -800.0) ? -800.0 : x;
  const double n = __builtin_rint(x * 1.44269504088896338700e+00);
  double r = fma(-n, 6.93147180369123816490e-01, x);       // ln2_hi = 0x3FE62E42FEE00000
  r = fma(-n, 1.90821492927058770002e-10, r);              // ln2_lo
  double p = 1.6059043836821613e-10;                        // 1/13!
  p = fma(p, r, 2.08767569878680989792e-09);                // 1/12!
  p = fma(p, r, 2.50521083854417187751e-08);                // 1/11!
  p = fma(p, r, 2.75573192239858906526e-07);                // 1/10!
  p = fma(p, r, 2.75573192239858906526e-06);                // 1/9!
  p = fma(p, r, 2.48015873015873015873e-05);                // 1/8!
  p = fma(p, r, 1.98412698412698412698e-04);                // 1/7!
  p = fma(p, r, 1.38888888888888888889e-03);                // 1/6!
  p = fma(p, r, 8.33333333333333333333e-03);                // 1/5!
  p = fma(p, r, 4.16666666666666666667e-02);                // 1/4!
  p = fma(p, r, 1.66666666666666666667e-01);                // 1/3!
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  // n is an integer-valued double or NaN; beyond int range the conversion saturates, which is still "result 0"
  return __builtin_amdgcn_ldexp(p, (int)fmax(n, -2147483000.0));
}
// 1 / sqrt(x) for x > 0 from the same refinement: 2 h closed by one Newton step against the refined root — ~1 ulp, where a raw
// v_rsq_f64 has about 26 good bits.  The Matern nu = 0.5 slope divides by r with it.
__device__ __forceinline__ double gpbo_rsqrt_pos(double x) {
  double g, h;
  gpbo_sqrt_refine(x, g, h);
  const double inv = h + h;
  return fma(inv, fma(-g, inv, 1.0), inv);
}
static_assert(GPBO_KERNEL_RBF == 0 && GPBO_KERNEL_MATERN25 == 1 && GPBO_KERNEL_MATERN15 == 2 && GPBO_KERNEL_MATERN05 == 3,
              "the kernel kinds of gpbo.h");
// Matern nu = 1.5 (kernels.py Matern.__call__): s = sqrt(3) r, k = (1 + s) exp(-s); nu = 0.5: k = exp(-r).  d2 = 0 gives exactly 1.
template <int KERNEL>
__device__ __forceinline__ double gpbo_kernel_value(double d2) {
  static_assert(KERNEL >= GPBO_KERNEL_RBF && KERNEL <= GPBO_KERNEL_MATERN05, "unknown kernel kind");
  if (KERNEL == GPBO_KERNEL_MATERN25) {
    const double k = gpbo_sqrt_pos(d2) * 2.23606797749978969641;
    return (1.0 + k + (k * k) * 0.33333333333333333333) * gpbo_exp_nonpos(-k);
  } else if (KERNEL == GPBO_KERNEL_MATERN15) {
    const double s = gpbo_sqrt_pos(d2) * 1.73205080756887729353;
    return (1.0 + s) * gpbo_exp_nonpos(-s);
  } else if (KERNEL == GPBO_KERNEL_MATERN05) {
    // An infinite distance (a +-inf coordinate) is exp(-inf) = 0, as sklearn has it; gpbo_sqrt_pos(inf) would be NaN (rsq(inf) = 0,
    // inf * 0), so the root sees 1e300 at most: exp(-1e150) is the same exact 0.  The comparison is false for NaN, which still
    // propagates.  (nu = 2.5 / 1.5 keep their NaN there: inf * exp(-inf) is NaN in NumPy too; RBF takes no root.)
    return gpbo_exp_nonpos(-gpbo_sqrt_pos(d2 > 1e300 ? 1e300 : d2));
  } else {
    return gpbo_exp_nonpos(-0.5 * d2);
  }
}
// The slope f(d2) of a kernel, given its value kv = gpbo_kernel_value<KERNEL>(d2) — the one factor both gradients are made of:
//   dk / dxs_t      =  f * (xs_t - Xs_t)      the gradient in the (scaled) inputs: posterior_small.hip, polish_fused.hip
//   dK / dlog l_t   = -f * (xs_t - Xs_t)^2    what the LML gradient accumulates: lml_bodies.h (kernels.py:1764-1766, 1567-1582)
//   RBF        f = -k
//   nu = 2.5   f = -(5/3) (1 + s) exp(-s), s = sqrt(5) r        (no 1 / r singularity)
//   nu = 1.5   f = -3 exp(-sqrt(3) r)                           (none either)
//   nu = 0.5   f = -exp(-r) / r for r > 0 and 0 at r = 0: sklearn zeroes the non-finite gradient entries of coincident points
//              (kernels.py: K_gradient[~np.isfinite(K_gradient)] = 0), so a candidate ON a training point gets no gradient from it.
// LIBM_ROOT: the nu = 2.5 root as sqrt(5 d2) through the library's square root, the arithmetic the LML gradient has had from its
// first version (its values are part of what a theta search returns); everywhere else the root is gpbo_sqrt_pos, as in the value.
template <int KERNEL, bool LIBM_ROOT = false>
__device__ __forceinline__ double gpbo_kernel_slope(double d2, double kv) {
  static_assert(KERNEL >= GPBO_KERNEL_RBF && KERNEL <= GPBO_KERNEL_MATERN05, "unknown kernel kind");
  if (KERNEL == GPBO_KERNEL_MATERN25) {
    if (LIBM_ROOT) {
      const double tmp = sqrt(5.0 * d2);
      return -(5.0 / 3.0 * (tmp + 1.0) * gpbo_exp_nonpos(-tmp));
    }
    const double s = gpbo_sqrt_pos(d2) * 2.23606797749978969641;      // sqrt(5) r
    return -1.66666666666666666667 * (1.0 + s) * gpbo_exp_nonpos(-s);
  } else if (KERNEL == GPBO_KERNEL_MATERN15) {
    return -3.0 * gpbo_exp_nonpos(-(gpbo_sqrt_pos(d2) * 1.73205080756887729353));
  } else if (KERNEL == GPBO_KERNEL_MATERN05) {
    return d2 > 0.0 ? -kv * gpbo_rsqrt_pos(d2) : 0.0;
  } else {
    return -kv;
  }
}
#endif

// Every writer of the candidate set (and every call that uses the candidate buffers for points of its own) ends the resident
// posteriors: none is valid (M_post) and none can be refreshed.
inline void drop_posteriors(gpbo_ctx* ctx) {
  for (auto& m : ctx->models) { m.M_post = -1; m.refreshable = false; }
}
inline void drop_refreshable(gpbo_ctx* ctx) {
  for (auto& m : ctx->models) m.refreshable = false;
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int pad_dim(int d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64; }

// Template instance dispatch of the posterior launchers: f(kernel) / f(dp, kernel) with std::integral_constant arguments for the
// model's kernel type (the four kinds of gpbo.h) and padded dimension (pad_dim's values).  A kind outside the four runs nothing:
// check_gp_args (gpbo_api.hip) lets none into a model, and one that got here anyway is an error, never a silent RBF.
template <typename F>
int with_kernel(gpbo_ctx* ctx, int kernel, F&& f) {
  switch (kernel) {
    case GPBO_KERNEL_RBF: return f(std::integral_constant<int, GPBO_KERNEL_RBF>{});
    case GPBO_KERNEL_MATERN25: return f(std::integral_constant<int, GPBO_KERNEL_MATERN25>{});
    case GPBO_KERNEL_MATERN15: return f(std::integral_constant<int, GPBO_KERNEL_MATERN15>{});
    case GPBO_KERNEL_MATERN05: return f(std::integral_constant<int, GPBO_KERNEL_MATERN05>{});
  }
  GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "unknown kernel kind " + std::to_string(kernel));
}
// every kind's instance in turn (the per-device function attributes of a kernel template)
template <typename F>
int for_each_kernel(gpbo_ctx* ctx, F&& f) {
  for (const int kernel : {GPBO_KERNEL_MATERN25, GPBO_KERNEL_RBF, GPBO_KERNEL_MATERN15, GPBO_KERNEL_MATERN05})
    if (const int rc = with_kernel(ctx, kernel, f)) return rc;
  return GPBO_OK;
}
// ... and the <KERNEL, WLDS> instances of the one-launch search kernels (search_plan.h: W in LDS or streamed from memory)
template <typename F>
int with_kernel_wlds(gpbo_ctx* ctx, int kernel, bool wlds, F&& f) {
  return with_kernel(ctx, kernel, [&](auto k) -> int { return wlds ? f(k, std::true_type{}) : f(k, std::false_type{}); });
}
template <typename F>
int for_each_kernel_wlds(gpbo_ctx* ctx, F&& f) {
  return for_each_kernel(ctx, [&](auto k) -> int {
    if (const int rc = f(k, std::true_type{})) return rc;
    return f(k, std::false_type{});
  });
}
template <typename F>
int with_dp_kernel(gpbo_ctx* ctx, int DP, int kernel, F&& f) {
  return with_kernel(ctx, kernel, [&](auto k) -> int {
    switch (DP) {
      case 4: return f(std::integral_constant<int, 4>{}, k);
      case 8: return f(std::integral_constant<int, 8>{}, k);
      case 16: return f(std::integral_constant<int, 16>{}, k);
      case 32: return f(std::integral_constant<int, 32>{}, k);
      case 64: return f(std::integral_constant<int, 64>{}, k);
    }
    GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "posterior: unsupported padded dimension");
  });
}

template <typename T>
int ensure(gpbo_ctx* ctx, T** p, int64_t* cap, int64_t need) {
  if (need <= *cap && *p) return GPBO_OK;
  if (*p) {
    GPBO_HIP(ctx, hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  void* q = nullptr;
  GPBO_HIP(ctx, hipMalloc(&q, (size_t)need * sizeof(T)));
  *p = (T*)q;
  *cap = need;
  return GPBO_OK;
}

// ---- launchers implemented in the kernel translation units ---------------------------------
// fit_kernels.hip
int launch_prescale(gpbo_ctx* ctx, const double* X, int64_t n, int d, int DP, const double* ls,
                    double* out, int64_t n_pad);
int launch_kmat(gpbo_ctx* ctx, Model& m, double noise, double* out);   // out: m.K, or m.L (factorised in place)
int launch_lane_targets(gpbo_ctx* ctx, const double* y, int64_t n, double* yn);   // scaled lanes: yn = y * ts_l per lane (ctx->lane_pair)
int launch_fill_w_diag(gpbo_ctx* ctx, Model& m, bool zero_fill = true);
int launch_trmv(gpbo_ctx* ctx, Model& m);
int launch_append_row(gpbo_ctx* ctx, Model& m, int64_t j);   // row j (== current m.N) from the prescaled m.Xs[j]
int launch_pack_w(gpbo_ctx* ctx, Model& m);
struct GemmArgs {
  int m, n, k;            // multiples of 64 / 64 / 16
  double alpha, beta;
  const double* A; int64_t lda; int64_t strideA;
  const double* B; int64_t ldb; int64_t strideB;
  double* C; int64_t ldc; int64_t strideC;
  int lanes = 1; int64_t lane_stride = 0;   // filled in by launch_gemm from the context (lane mode)
  int batch;
  int b_trans;            // B given as (n,k) row-major
  int lower_only;         // skip output tiles strictly above the diagonal (m == n)
  int a_lower;            // A is lower triangular (k == m): k-loop stops at the row tile's diagonal
  int b_lower;            // B is lower triangular (k == n, not transposed): k-loop starts at the column tile
  int a_trans;            // A given as (k,m) row-major (C = A^T B)
  int k_from_tile;        // k-loop starts at max(row tile, column tile): W^T W with W lower triangular
  int tri_grid;           // set by launch_gemm: blockIdx.x = linear lower-triangle index of the output tile (lower_only products)
  int skip00;             // leave the leading skip00 x skip00 output tiles alone (64x64-tile kernel only): the diagonal-block
                          // workgroup of the same launch (or an earlier launch) owns them
  int fat;                // 0: launch_gemm decides from this product's shape whether the sixteen-wave tile kernel takes it (another
                          // summation order over k, i.e. other bits); +1 / -1: the caller has decided — a product that one code path
                          // launches whole and another in pieces (the Cholesky's trailing updates) must come out the same either way
};
int launch_gemm(gpbo_ctx* ctx, const GemmArgs& g);
// launch_gemm's own rule for g.fat == 0 (exposed for callers that split a product)
bool gemm_fat_rule(const GemmArgs& g);
// chol_kernels.hip: blocked Cholesky of m.L in place + inverted 64x64 diagonal blocks (128-column steps, `outer`-column panels);
// stamps (device, >= 8 words, may be null): in-kernel clocks of the first diagonal workgroup
int launch_cholesky128(gpbo_ctx* ctx, Model& m, int outer, long long* stamps);
// fused_small.hip: the fit (mode 0: ... + packed W) or an LML evaluation (1: value, 2: value + gradient; noise_grad: + the noise
// component g_eta behind the length scales' — scaled_kernel.h) of m (and, in lane mode, of
// ctx->lanes models) as ONE launch; src 0: raw X / y / ls_in given (device-visible), 1: m.Xs / m.yn / m.ls resident.  The pivot word
// and the LML scalars land in the device-visible host words info_out / out (pitches per lane, in ints / doubles).
int fused_max_np();
int launch_fused_small(gpbo_ctx* ctx, Model& m, int mode, int src, int n_ls, const double* X, const double* y, const double* ls_in,
                       double* scal, int* info_out, int64_t info_pitch, double* out, int64_t out_pitch, bool noise_grad = false);
// mid_fit.hip: the strip path's launches (lane-aware through ctx->lanes / lane_stride)
int mid_max_np();
int launch_mid_inputs(gpbo_ctx* ctx, Model& m, const double* X, const double* y, const double* ls_in);
int launch_kmat_q(gpbo_ctx* ctx, Model& m, double noise, double* out);
int launch_w_strip(gpbo_ctx* ctx, Model& m, bool pack);                                   // W, the strips' share of W y (m.tmp), Wp if pack
int launch_alpha_strip(gpbo_ctx* ctx, Model& m, int* info_out, int64_t info_pitch);     // alpha; pivot word -> info_out (device-visible host word)
// posterior_kernel.hip
int launch_posterior(gpbo_ctx* ctx, Model& m, int64_t M, double y_mean, double y_std);
int launch_posterior_grad(gpbo_ctx* ctx, Model& m, int64_t M, double y_mean, double y_std, double** dmu_dev, double** dsd_dev,
                          double** packed_dev = nullptr,    // packed: [dmu | dsd | mu | sd] contiguous (mu / sd not in the model's buffers)
                          const double* xc_in = nullptr,    // the points (M, d), device-visible, instead of the resident candidate set
                          double* packed_out = nullptr);    // where the packed block goes (device-visible) instead of ctx->mu_part
// posterior_kernel_v2.hip
// Both ends of a posterior pass inside the fused kernel's launch (round 6), when ONE workgroup owns every row of its candidates
// (one row chunk): the candidate tile is scaled on its way into LDS (prescale_elem's division: no prescale launch, no scaled
// image in memory) and the epilogue writes mu and sd itself (posterior_finalize_elem: no partials, no finalize launch).
struct PostEnds {
  const double* Xc;     // raw candidates [M][d]
  const double* ls;     // length scales [d]
  int d;
  int64_t M;
  double y_mean, y_std;
  double amplitude, white;   // of the model (1, 0 unless it is a scaled one)
  double* mu;
  double* sd;
  int* negvar;
};
// The launchers of the paths (PostPath: posterior_plan.h); plan_posterior sizes their grids and ctx->part / ctx->mu_part.
int launch_posterior_fused(gpbo_ctx* ctx, Model& m, int64_t Mp, const PostPlan& plan, const PostEnds& ends);   // Fused256, Fused512
// The slab paths (the walk: posterior_kernel.hip): the k* slab of candidates [m0, m0 + ldk) as fp64 values, fp32 values or int8
// digit planes (+ the partial means) ...
int launch_kstar_slab(gpbo_ctx* ctx, Model& m, double* Kst, int64_t ldk, int64_t Mp, int64_t m0, int nchunks);
int launch_kstar_slab_f32(gpbo_ctx* ctx, Model& m, float* Kst, int64_t ldk, int64_t Mp, int64_t m0, int nchunks);
int launch_kstar_digits(gpbo_ctx* ctx, Model& m, void* Kd, int64_t ldk, int64_t Mp, int64_t m0, int nchunks);
// ... and each path's GEMM over that slab: the partial sums of squares of candidates [m0, m0 + ldk) into ctx->part [part_chunks][Mp]
int launch_slab_gemm_f64(gpbo_ctx* ctx, Model& m, const double* slab, int64_t ldk, int64_t m0, int64_t Mp, int part_chunks);
int launch_slab_gemm_f32(gpbo_ctx* ctx, Model& m, const float* slab, int64_t ldk, int64_t m0, int64_t Mp, int part_chunks);   // posterior_kernel_f32.hip
int launch_slab_gemm_i8(gpbo_ctx* ctx, Model& m, const void* slab, int64_t ldk, int64_t m0, int64_t Mp, int part_chunks);      // posterior_i8.hip
int prepare_posterior_i8(gpbo_ctx* ctx, Model& m);   // before the first int8 slab: W's digit planes (once per fit), the device's compute units
// posterior_refresh.hip: the resident mu / sd of m brought from m.N_post to m.N rows (gpbo_posterior_refresh's incremental route)
int launch_posterior_refresh(gpbo_ctx* ctx, Model& m, int64_t M, double y_mean, double y_std);
// posterior_paths.hip: the negated values of n_paths posterior function draws over the M resident candidates into ctx->ys [n_paths][M].
// The call's workspace (path_plan.h: path_block, with room for n_runs ascent runs behind V; 0: none) is handed back in *ws.
struct PathWorkspace { double* base; PathBlock at; double* p(int64_t off) const { return base + off; } };   // base = ctx->paths
int launch_sample_paths(gpbo_ctx* ctx, const Model& m, int64_t M, double y_mean, double y_std, int n_paths, int n_features,
                        const double* omega, const double* phase, const double* weights, const double* eps, int n_runs,
                        PathWorkspace* ws);
// gpbo_sample_paths_constrained: one slot's pass with its epilogue (path_plan.h: PathEpilogue), and the last pass's paths again at
// up to 16 candidates (the picks of the rows without a feasible candidate)
struct PathFold { int epilogue; double lb, ub; double* viol; double* vals; };
int launch_sample_paths_fold(gpbo_ctx* ctx, const Model& m, int64_t M, double y_mean, double y_std, int n_paths, int n_features,
                             const double* omega, const double* phase, const double* weights, const double* eps, const PathFold& fold,
                             PathWorkspace* ws);
int launch_paths_at(gpbo_ctx* ctx, const Model& m, const PathWorkspace& ws, double y_mean, double y_std, int n_paths, int n_features,
                    const int64_t* idx, int n, double* pts, double* f, int ld);
// ... the workspace's draws at n points of the caller's (P [>= n][DP], scaled, on the device): out[s * ld + r] = f_s(P_r), the plain store
int launch_paths_over(gpbo_ctx* ctx, const Model& m, const PathWorkspace& ws, double y_mean, double y_std, int n_paths, int n_features,
                      const double* P, int64_t n, double* out, int64_t ld);
// ... the same with an epilogue (PathFold) behind the accumulators instead of the plain store; fold.viol / fold.vals have out's ld
int launch_paths_over_fold(gpbo_ctx* ctx, const Model& m, const PathWorkspace& ws, double y_mean, double y_std, int n_paths,
                           int n_features, const double* P, int64_t n, double* out, int64_t ld, const PathFold& fold);
// ... and the first half of it alone: the draws' inputs and V = alpha - W^T (W (g(X) + eps)) made resident, no candidates needed
int launch_path_weights(gpbo_ctx* ctx, const Model& m, int n_paths, int n_features, const double* omega, const double* phase,
                        const double* weights, const double* eps, int n_runs, PathWorkspace* ws);
// ... and the solve inside it: V[s] = a - W^T (W (G[s] + eps[s])), S columns (G, T, V [S][NP], eps [S][N], a [NP]; all on the device)
int launch_path_solve(gpbo_ctx* ctx, const Model& m, int S, const double* G, const double* eps, const double* a, double* T, double* V);
// path_ascent.hip: gpbo_ascend_paths' runs, n_paths x n_starts workgroups in one launch, from host starts (n_paths n_starts, d) or —
// starts null — from the rows start_idx (local indices, host) of the resident candidates; ws was laid out for n_runs =
// n_paths * n_starts.  Synchronises.
int launch_path_ascent(gpbo_ctx* ctx, const Model& m, const PathWorkspace& ws, int n_paths, int n_starts, int n_features,
                       double y_mean, double y_std, const double* starts, const int64_t* start_idx, const double* box_lo,
                       const double* box_hi, int max_iter, double* x_out, double* f_out, double* g_out, int* status_out,
                       int* eval_out);
// posterior_cov.hip
int launch_posterior_cov(gpbo_ctx* ctx, Model& m, int64_t M, double y_std, double** cov_dev, int64_t* ld_cov);
// posterior_kernel_f32.hip
int launch_pack_w32(gpbo_ctx* ctx, Model& m);
// acq_kernels.hip
struct AcqArgs {
  int acq; double param; double y_max; int n_constraints;
  double lb[GPBO_MAX_MODELS]; double ub[GPBO_MAX_MODELS];
  const double* mu[GPBO_MAX_MODELS]; const double* sd[GPBO_MAX_MODELS];
};
int launch_acq_argbest(gpbo_ctx* ctx, const AcqArgs& a, int64_t M, int k_seeds, int64_t offset,
                       int64_t* best_idx, double* best_val, int64_t* seed_idx, double* seed_val);
// acq_kernels.hip: the selection's sort key and its device record.  Key = (value, index) with NaN greater than everything (NumPy
// sorts NaN last) and -0.0 == 0.0; ties break to the lowest index.
struct Key {
  double v;
  int64_t i;
};
struct SelState {     // lives in device memory, carried from pass to pass
  Key prev;           // last pick (i = -1 before the first pass)
  int64_t first_nan;  // lowest index holding NaN (INT64_MAX if none)
};
// acq_kernels.hip: launch_values_argbest's selection of ONE pick over ctx->ys[0..M) enqueued on ctx->stream and nothing fetched:
// *st_out / *pick_out are the device record (the arg-best is st->first_nan where that is not INT64_MAX, else *pick_out)
int enqueue_values_select(gpbo_ctx* ctx, int64_t M, const SelState** st_out, const Key** pick_out);
// acq_kernels.hip: launch_acq_argbest's selection and outputs over the values already in ctx->ys[0..M); synchronises
int launch_values_argbest(gpbo_ctx* ctx, int64_t M, int k_seeds, int64_t offset, int64_t* best_idx, double* best_val,
                          int64_t* seed_idx, double* seed_val);
// mes.hip: ctx->ys[i] = -a(x_i), the negated max-value entropy search value of the M resident candidates from m's resident mu / sd
// and n_samples <= GPBO_MAX_MES_SAMPLES sampled maxima y_star (host; they travel in the kernel's arguments)
int launch_mes_values(gpbo_ctx* ctx, const Model& m, int64_t M, int n_samples, const double* y_star);
// kg.hip: ctx->ys[i] = -KG(x_i), the negated knowledge gradient of the M resident candidates over themselves and the J reference
// points `points` (J, d; host, parameter space) from m's resident mu / sd; mu_points_out (J,; host) or null.  The caller has checked
// every argument.  The call's workspace is ctx->kg (kg.hip: kg_block).
int launch_kg_values(gpbo_ctx* ctx, const Model& m, int64_t M, const double* points, int J, double y_mean, double y_std,
                     double* mu_points_out);
// ehvi.hip: ctx->ys[i] = -EHVI(x_i), the negated expected hypervolume improvement of the M resident candidates from the resident
// mu / sd of slots 0 .. n_obj - 1, the level rows `levels` (n_obj, GPBO_MAX_EHVI_LEVELS) and the boxes cell_lo / cell_hi (n_cells, n_obj)
// of level indices (all host).  The caller has checked every argument.  The call's workspace is ctx->ehvi.
int launch_ehvi_values(gpbo_ctx* ctx, int n_obj, int64_t M, const int* n_levels, const double* levels, int64_t n_cells,
                       const uint8_t* cell_lo, const uint8_t* cell_hi);
// qnei.hip: gpbo_qnei_greedy behind its argument checks (include/gpbo.h has the formulas; qnei_plan.h the workspace, in ctx->greedy)
int launch_qnei_greedy(gpbo_ctx* ctx, const Model& m, int64_t M, double y_mean, double y_std, int n_groups, int n_paths, int n_features,
                       const double* omega, const double* phase, const double* weights, const double* eps, int noisy, double y_best,
                       const double* pending, int n_pending, int q, int64_t index_offset, int64_t* pick_idx, double* pick_gain,
                       double* baseline_out, double* values_out, double* keys_out);
// qnei.hip: gpbo_cnei_greedy behind its argument checks (include/gpbo.h has the rule; cnei_plan.h the workspace, in ctx->greedy): ms /
// y_mean / y_std per slot 0 .. C, lb / ub per constraint, the draws' inputs concatenated slot-major, then group-major
int launch_cnei_greedy(gpbo_ctx* ctx, int n_constraints, const Model* const* ms, int64_t M, const double* y_mean, const double* y_std,
                       const double* lb, const double* ub, int n_groups, int n_paths, int n_features, const double* omega,
                       const double* phase, const double* weights, const double* eps, double y_floor, const double* base, int n_base,
                       int q, int64_t index_offset, int64_t* pick_idx, double* pick_gain, double* pick_feasible, double* baseline_out,
                       double* values_out, double* viol_out, double* base_values_out, double* keys_out);
// qnehvi.hip: gpbo_qnhvi_greedy behind its argument checks (include/gpbo.h has the formulas; qnehvi_plan.h the workspace,
// in ctx->greedy): ms / y_mean / y_std per objective, the draws' inputs concatenated in slot order
int launch_qnehvi_greedy(gpbo_ctx* ctx, const Model* const* ms, int64_t M, const double* y_mean, const double* y_std, int n_groups,
                         int n_paths, int n_features, const double* omega, const double* phase, const double* weights,
                         const double* eps, const double* ref, const double* base, int n_base, int q, int64_t index_offset,
                         int64_t* pick_idx, double* pick_gain, int* front_size_out, double* fronts_out, double* values_out,
                         double* base_values_out, double* keys_out);
// ehvi.hip: gpmo_cehvi_argbest's values (include/gpmo.h): launch_ehvi_values' EHVI weighted by the feasibility of the constraints in
// slots n_obj .. n_obj + n_constraints - 1, in the same kernel: ctx->ys[i] = -(E exp(s)) (log_form == 0) or -(log E + s)
int launch_cehvi_values(gpbo_ctx* ctx, int n_obj, int64_t M, const int* n_levels, const double* levels, int64_t n_cells,
                        const uint8_t* cell_lo, const uint8_t* cell_hi, int n_constraints, const double* lb, const double* ub,
                        int log_form);
// qnehvi.hip: gpmo_cnhvi_greedy behind its argument checks (include/gpmo.h has the rule; cmo_plan.h the workspace, in ctx->greedy):
// ms / y_mean / y_std per slot (the two objectives, then the C constraints), the draws' inputs concatenated slot-major, then group-major
int launch_cnhvi_greedy(gpbo_ctx* ctx, int n_constraints, const Model* const* ms, int64_t M, const double* y_mean, const double* y_std,
                        const double* lb, const double* ub, int n_groups, int n_paths, int n_features, const double* omega,
                        const double* phase, const double* weights, const double* eps, const double* ref, const double* base,
                        int n_base, int q, int64_t index_offset, int64_t* pick_idx, double* pick_gain, double* pick_feasible,
                        int* front_size_out, double* fronts_out, double* values_out, double* viol_out, double* base_values_out,
                        double* keys_out);
#ifdef GPBO_DEBUG
int debug_qnehvi_fronts(gpbo_ctx* ctx, int T, int n, const double* base_values, const double* ref, int n_insert,
                        const double* insert_values, int* front_size_out, double* fronts_out);
int debug_kg_lines(gpbo_ctx* ctx, const double* a, const double* b, int64_t R, int n_lines, double* out);
int debug_kg_stage_ms(gpbo_ctx* ctx, float* ms3);
#endif
// trust_region.hip: debug build: records event i (0 before, 1 after) of a candidate generator's kernel for gpbo_debug_generate_ms;
// the product records nothing
void generate_mark(gpbo_ctx* ctx, int i);
// acq_kernels.hip: the k best of each of n_rows rows of M keys (rows + r * ld), the rules of launch_acq_argbest: best_idx / best_val
// (n_rows) the arg-best, top_idx (n_rows, k; may be null) the rows' k smallest keys in order (ties to the lowest index, NaNs last)
// as LOCAL indices; synchronises
int launch_topk_rows(gpbo_ctx* ctx, double* rows, int64_t ld, int n_rows, int64_t M, int k, int64_t offset, int64_t* best_idx,
                     double* best_val, int64_t* top_idx);
// (value, global index) records of one shard, as they travel between GPUs: record 0 = the arg-best (value NaN: "my
// first NaN sits at this index"), records 1..k = argsort[:k] (index -1 = padding)
struct BestRecord { double v; int64_t i; };
// acq + selection enqueued on ctx->stream, the 1 + k_seeds records left ON THE DEVICE at `records_dev`
int launch_acq_records(gpbo_ctx* ctx, const AcqArgs& a, int64_t M, int k_seeds, int64_t offset, BestRecord* records_dev);
// gpbo_debug_select: the selection launches alone over caller-supplied values (variant 1: k passes, 2: threshold + ranks), timed
int debug_select(gpbo_ctx* ctx, const double* ys_host, int64_t M, int k, int variant, int iters, int64_t* idx_out, double* val_out,
                 int64_t* first_nan_out, float* ms_out);
// the reference's argmin / min / argsort[:k] over the union of `world` shards from their records (host; identical on every rank)
void merge_records(const BestRecord* all, int world, int k_seeds, int64_t* best_idx, double* best_val, int64_t* seed_idx,
                   double* seed_val);
// gpbo_api.hip: the theta search's raw inputs made resident on ctx's device (gpbo_lml_batch with X == NULL reads them)
int lml_upload_inputs(gpbo_ctx* ctx, const double* X, const double* y_norm, int64_t N, int d);
// gpbo_api.hip: argument checks + posterior pointers of gpbo_acq_argbest, shared with the multi-GPU entry points
int build_acq_args(gpbo_ctx* ctx, const char* who, int acq, double acq_param, double y_max, int n_constraints,
                   const double* lb, const double* ub, int k_seeds, const void* best_idx, const void* best_val,
                   const void* seed_idx, const void* seed_val, AcqArgs* out);
// posterior_small.hip
int launch_posterior_small(gpbo_ctx* ctx, Model& m, int M, double y_mean, double y_std);
int small_batch_limit(int64_t NP);   // largest M the GEMV path takes (posterior_small.hip)
// polish_fused.hip: gpbo_polish_seeds' runs as one launch (one workgroup per run) by the caller's plan (search_plan.h: plan_polish,
// a served mode).  The seeds and the box go in and the results land in ctx->polish_pinned, a device-visible block of at least
// block.bytes laid out by `block` (polish_block(n_seeds, d)).  eval_repeat = R > 0: no search, R evaluations at every seed (the debug
// entry's timing and parity seam).
int launch_polish_fused(gpbo_ctx* ctx, Model& m, const PolishPlan& plan, const PolishBlock& block, int acq, double acq_param,
                        double y_max, double y_mean, double y_std, const double* seeds, int n_seeds, const double* box_lo,
                        const double* box_hi, int max_iter, int eval_repeat);
int launch_posterior_grad_small(gpbo_ctx* ctx, Model& m, int M, double y_mean, double y_std, double* dmu_dev, double* dsd_dev,
                                double* mu_out, double* sd_out);
// lml_kernels.hip
// (out / grad: lane l's words l * out_pitch doubles behind lane 0's — device memory or device-visible pinned host words)
int launch_lml_terms(gpbo_ctx* ctx, Model& m, double* out2, int64_t out_pitch);
int launch_lml_grad(gpbo_ctx* ctx, Model& m, int n_ls, const double* Kinv, double* partial, double* out, int64_t out_pitch,
                    bool with_terms,    // out[2..] = gradient; with_terms: out[0], out[1] too (launch_lml_terms' job, same arithmetic)
                    bool noise_grad = false);   // out[2 + n_ls] = g_eta = 0.5 (|alpha|^2 - tr K^-1), the component for dK / dtheta = I
// comm.hip: ncclCommCount of the context's communicator (0: none, -1: not answered)
int comm_nranks(gpbo_ctx* ctx);
// mt_jump.hip: states_dev[w] = block 1 + poly_idx[w] * stride_blocks of the MT19937 sequence whose block 0 is key_dev
int mt_jump_states(gpbo_ctx* ctx, const unsigned* key_dev, int64_t stride_blocks, int max_k, const int* poly_idx_dev,
                   int n_states, unsigned* seq_dev, unsigned* states_dev, unsigned* windows_dev);
// probe.hip
int run_mfma_peak(gpbo_ctx* ctx, int iters, double* tflops);
int run_copy_peak(gpbo_ctx* ctx, int64_t bytes, double* gbps);
int run_mfma_probe(gpbo_ctx* ctx, int iters, int waves_per_simd, int mode, double* out4);
#ifdef GPBO_DEBUG
int run_hybrid_probe(gpbo_ctx* ctx, int iters, int cfg, double* out3);
// latency_probe.hip (debug build only: the one kernel of the library that uses scratch)
int run_latency_probe(gpbo_ctx* ctx, long long* out_host, int n);
#endif

inline void ev_begin(gpbo_ctx* ctx, int slot) {
  if (ctx->no_timing || ctx->timing_off) return;
  EventPair& e = ctx->ev[slot];
  if (!e.a) { (void)hipEventCreate(&e.a); (void)hipEventCreate(&e.b); }
  (void)hipEventRecord(e.a, ctx->stream);
  e.used = false;
}
inline void ev_end(gpbo_ctx* ctx, int slot) {
  if (ctx->no_timing || ctx->timing_off) return;
  EventPair& e = ctx->ev[slot];
  (void)hipEventRecord(e.b, ctx->stream);
  e.used = true;
}

}  // namespace gpbo
