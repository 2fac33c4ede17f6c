// Expected hypervolume improvement over the resident candidates (gfx950): gpbo_ehvi_argbest's values.  m = 2 or 3 objectives, all
// maximised, independent posteriors Y_j ~ N(mu_j(x), sd_j(x)^2) from slots 0 .. m - 1; the region not dominated by the front and
// above the reference point comes as K disjoint boxes [l_k, u_k) whose bounds along objective j are entries of objective j's level
// list (include/gpbo.h has the inputs and the conventions):
//   g_j(a)  = E[(Y_j - a)^+] = sd_j f((mu_j - a) / sd_j),   f(z) = phi(z) + z Phi(z),   g_j(+inf) = 0
//   EHVI(x) = sum_k prod_j (g_j(l_kj) - g_j(u_kj))
//   ys[i]   = -EHVI(x_i)                          the key the selection launches of acq_kernels.hip minimise
// Compiled with -ffp-contract=off, as acq_kernels.hip: acq_formulas.h's pieces give the bits they give there.
//
// f over its two ranges:
//   z > -1    as written, ndtr_dev / norm_pdf_dev.
//   z <= -1   phi(z) r(z), r = log_ei_ratio(z) = 1 + z Phi / phi (erfcx down to -28, the series below): the form GPBO_ACQ_LOG_EI takes
//             the logarithm of.  The sum as written cancels there; this one keeps a candidate far below the front relatively accurate
//             and correctly ordered.  Where phi underflows to 0 (z < ~ -38.6, and the +inf level) the factor is 0.
//
// Two stages per tile of C candidates, one workgroup of 512 threads = G = 512 / C groups of C lanes (c = thread % C, g = thread / C):
//   tables   tab[(j Lmax + l) C + c] = g_j(levels[j][l]) of candidate c, in LDS — every level ONCE per candidate, not once per cell.
//            A per-thread table indexed by a cell's level number would sit in scratch memory.  Candidate-minor: the lanes of a wave
//            read consecutive doubles for one level index, every bank once.  Group g fills levels g, g + G, ... of each objective.
//   cells    group g sums its chunk of the cell list, lane c for candidate c: per cell m pairs of LDS reads, m subtractions,
//            m - 1 multiplications, one addition.  A cell is ONE 8-byte word (byte j: lo_j, byte 3 + j: hi_j), the same for every lane
//            of a group; with C >= 64 a wave lies inside one group and the word is a scalar load.
//
// The tile rule (ehvi_tile): with T = m Lmax, Lmax the largest level count, C is the largest of 256, 128, 64, 32 whose tables fit the
// 160 KiB of LDS a workgroup may take, T C 8 <= 163840:
//   T <= 80 -> C = 256 (G = 2)     T <= 160 -> C = 128 (G = 4)     T <= 320 -> C = 64 (G = 8)     else C = 32 (G = 16; T <= 390)
// (m = 2: Lmax 40 | 41 and 80 | 81; m = 3: Lmax 26 | 27, 53 | 54 and 106 | 107.)  The cell list is cut into G chunks of
// P = ceil(K / G) cells, chunk g = [g P, min(K, (g + 1) P)): K is on a chunk boundary where it is a multiple of G, and with K < G some chunks are empty.
// 512 threads, not 256: the tables leave room for ONE workgroup per compute unit, and two waves per SIMD instead of one took the
// kernel from 0.88 / 2.48 / 40.9 ms to 0.70 / 1.76 / 22.1 ms (profiles/ehvi_bench.json's three cases); 1024 threads cap a wave at 128
// VGPRs and the C = 32 instances spill.
//
// THE ORDER OF THE SUM: each chunk runs k ascending into one accumulator that starts at 0; the chunk sums are then added
// g = 0 .. G - 1 in that order into one accumulator that starts at chunk 0's sum.  C, G and P are functions of m, the level counts
// and K alone: a candidate's bits depend neither on M, nor on the grid, nor on the other candidates.  fp64 whatever a slot's precision.
//
// gpmo_cehvi_argbest (include/gpmo.h) is the same kernel body with an epilogue: behind the box sum the lane that holds a candidate's
// EHVI E — the bits above — forms s = sum_j log p_j from the constraint slots' resident (cm, cs), j ascending into one accumulator
// from 0, by GPBO_ACQ_LOG_FEAS's function (acq_formulas.h: log_interval_dev), and stores -(E exp(s)) or -(log E + s).  Once per
// candidate, nothing through HBM, no second pass.  FORM = 0 is gpbo_ehvi_argbest's instance: its kernel keeps its name, its
// arguments and its code.
#include "gpbo_internal.h"
#include "acq_formulas.h"

#include <cmath>
#include <vector>

namespace gpbo {

constexpr int EHVI_THREADS = 512;
constexpr int EHVI_LDS_BYTES = 160 * 1024;

// candidates per workgroup from T = m * (largest level count)
static int ehvi_tile(int T) {
  for (int C = 256; C > 32; C /= 2)
    if ((int64_t)T * C * (int64_t)sizeof(double) <= EHVI_LDS_BYTES) return C;
  return 32;
}
static_assert((int64_t)GPBO_MAX_EHVI_OBJECTIVES * GPBO_MAX_EHVI_LEVELS * 32 * sizeof(double) <= EHVI_LDS_BYTES, "the smallest tile fits");

struct EhviDev {
  const double* mu[GPBO_MAX_EHVI_OBJECTIVES];
  const double* sd[GPBO_MAX_EHVI_OBJECTIVES];
  const double* levels;               // [m][GPBO_MAX_EHVI_LEVELS]
  const unsigned long long* cells;    // [K]: byte j = lo_j, byte 3 + j = hi_j
  int n_levels[GPBO_MAX_EHVI_OBJECTIVES];
  int l_max;                          // the tables' row stride per objective: the largest level count
  int n_cells, per_group;             // K, P
  int64_t M;
};

// gpmo_cehvi_argbest's constraints: slot m + j's resident posterior and bounds, j < n
struct EhviFeas {
  int n;
  const double* cm[GPBO_MAX_MODELS];
  const double* cs[GPBO_MAX_MODELS];
  double lb[GPBO_MAX_MODELS], ub[GPBO_MAX_MODELS];
};
enum EhviForm : int { EHVI_PLAIN = 0, EHVI_PRODUCT = 1, EHVI_LOG = 2 };

// g(a) = E[(Y - a)^+], Y ~ N(mean, sd^2); sd == 0: (mean - a)^+.  The caller has dealt with a NaN mean or sd.
__device__ __forceinline__ double ehvi_g_dev(double mean, double sd, double a) {
  if (sd == 0.0) {
    const double diff = mean - a;
    return diff > 0.0 ? diff : 0.0;
  }
  const double z = (mean - a) / sd;
  if (z > -1.0) return sd * (norm_pdf_dev(z) + z * ndtr_dev(z));
  const double pdf = norm_pdf_dev(z);
  if (pdf == 0.0) return 0.0;
  return sd * (pdf * log_ei_ratio(z, DevErfcx()));
}

template <int C, int NOBJ, int FORM>
__device__ __forceinline__ void ehvi_body(const EhviDev& a, const EhviFeas* __restrict__ feas, double* __restrict__ ys) {
  extern __shared__ __attribute__((aligned(16))) double ehvi_tab[];
  constexpr int G = EHVI_THREADS / C;
  const int c = threadIdx.x % C;
  // with C >= 64 a wave lies inside one group: its number is the same in every lane, and so is every cell word it loads
  const int g = C >= 64 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / C) : (int)threadIdx.x / C;
  const int64_t tiles = (a.M + C - 1) / C;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * C + c;
    const bool live = i < a.M;
    bool is_nan = false;
#pragma unroll
    for (int j = 0; j < NOBJ; ++j) {
      const double mean = live ? a.mu[j][i] : 0.0, sd = live ? a.sd[j][i] : 0.0;
      is_nan = is_nan || mean != mean || sd != sd;
      const double* lv = a.levels + j * GPBO_MAX_EHVI_LEVELS;
      double* col = ehvi_tab + (size_t)j * a.l_max * C + c;
      for (int l = g; l < a.n_levels[j]; l += G) col[(size_t)l * C] = live ? ehvi_g_dev(mean, sd, lv[l]) : 0.0;
    }
    __syncthreads();
    const int k0 = g * a.per_group;
    const int k1 = k0 + a.per_group < a.n_cells ? k0 + a.per_group : a.n_cells;
    double acc = 0.0;
#pragma unroll 4      // four cell words per load; the additions keep their order
    for (int k = k0; k < k1; ++k) {
      const unsigned long long w = a.cells[k];
      double p = 0.0;
#pragma unroll
      for (int j = 0; j < NOBJ; ++j) {
        const int lo = (int)((w >> (8 * j)) & 0xffu), hi = (int)((w >> (8 * (3 + j))) & 0xffu);
        const double* col = ehvi_tab + (size_t)j * a.l_max * C + c;
        const double f = col[(size_t)lo * C] - col[(size_t)hi * C];
        p = j == 0 ? f : p * f;
      }
      acc = acc + p;
    }
    if (G > 1) {
      __syncthreads();                       // every group is done with the tables: their first 512 words carry the chunk sums
      ehvi_tab[g * C + c] = acc;
      __syncthreads();
      if (g == 0)
        for (int q = 1; q < G; ++q) acc = acc + ehvi_tab[q * C + c];
    }
    if (g == 0 && live) {
      double key = -acc;
      if (FORM != EHVI_PLAIN) {
        double s = 0.0;
        for (int j = 0; j < feas->n; ++j) s = s + log_interval_dev(feas->lb[j], feas->ub[j], feas->cm[j][i], feas->cs[j][i]);
        key = FORM == EHVI_PRODUCT ? -(acc * exp(s)) : -(log(acc) + s);
      }
      ys[i] = is_nan ? NAN : key;
    }
    __syncthreads();                         // the next tile overwrites the tables
  }
}

template <int C, int NOBJ>
__global__ __launch_bounds__(EHVI_THREADS) void ehvi_kernel(EhviDev a, double* __restrict__ ys) {
  ehvi_body<C, NOBJ, EHVI_PLAIN>(a, nullptr, ys);
}

template <int C, int NOBJ, int FORM>
__global__ __launch_bounds__(EHVI_THREADS) void cehvi_kernel(EhviDev a, EhviFeas feas, double* __restrict__ ys) {
  ehvi_body<C, NOBJ, FORM>(a, &feas, ys);
}

constexpr int64_t EHVI_MAX_BLOCKS = 8192;     // the tile loop takes the rest

// debug build: an event before and after the value kernel of the last call (gpbo_debug_ehvi_ms); the product records nothing
static inline void ehvi_mark(gpbo_ctx* ctx, int i) {
#ifdef GPBO_DEBUG
  if (!ctx->ehvi_ev[i]) (void)hipEventCreate(&ctx->ehvi_ev[i]);
  (void)hipEventRecord(ctx->ehvi_ev[i], ctx->stream);
  ctx->ehvi_ev_used = (i == 1);
#else
  (void)ctx; (void)i;
#endif
}

// feas == nullptr: gpbo_ehvi_argbest's kernel; else the constrained one in product (log_form == 0) or log form
template <int C, int NOBJ>
static int ehvi_launch(gpbo_ctx* ctx, const EhviDev& a, size_t lds, const EhviFeas* feas, int log_form) {
  const int64_t tiles = (a.M + C - 1) / C;
  const dim3 grid((unsigned)(tiles < EHVI_MAX_BLOCKS ? tiles : EHVI_MAX_BLOCKS)), block(EHVI_THREADS);
  ehvi_mark(ctx, 0);
  if (!feas) ehvi_kernel<C, NOBJ><<<grid, block, lds, ctx->stream>>>(a, ctx->ys);
  else if (log_form) cehvi_kernel<C, NOBJ, EHVI_LOG><<<grid, block, lds, ctx->stream>>>(a, *feas, ctx->ys);
  else cehvi_kernel<C, NOBJ, EHVI_PRODUCT><<<grid, block, lds, ctx->stream>>>(a, *feas, ctx->ys);
  GPBO_HIP(ctx, hipGetLastError());
  ehvi_mark(ctx, 1);
  return GPBO_OK;
}

template <int NOBJ>
static int ehvi_launch_tile(gpbo_ctx* ctx, const EhviDev& a, int C, size_t lds, const EhviFeas* feas, int log_form) {
  switch (C) {
    case 256: return ehvi_launch<256, NOBJ>(ctx, a, lds, feas, log_form);
    case 128: return ehvi_launch<128, NOBJ>(ctx, a, lds, feas, log_form);
    case 64: return ehvi_launch<64, NOBJ>(ctx, a, lds, feas, log_form);
    default: return ehvi_launch<32, NOBJ>(ctx, a, lds, feas, log_form);
  }
}

// the tables take up to 160 KiB, past the 64 KiB a workgroup gets without asking (a per-device setting: once per context)
static int ehvi_lds_attr(gpbo_ctx* ctx) {
  if (ctx->func_attrs & ATTR_EHVI) return GPBO_OK;
  const void* kernels[] = {
      reinterpret_cast<const void*>(ehvi_kernel<256, 2>), reinterpret_cast<const void*>(ehvi_kernel<128, 2>),
      reinterpret_cast<const void*>(ehvi_kernel<64, 2>),  reinterpret_cast<const void*>(ehvi_kernel<32, 2>),
      reinterpret_cast<const void*>(ehvi_kernel<256, 3>), reinterpret_cast<const void*>(ehvi_kernel<128, 3>),
      reinterpret_cast<const void*>(ehvi_kernel<64, 3>),  reinterpret_cast<const void*>(ehvi_kernel<32, 3>)};
  for (const void* k : kernels) GPBO_HIP(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, EHVI_LDS_BYTES));
  ctx->func_attrs |= ATTR_EHVI;
  return GPBO_OK;
}
// ... and the constrained instances', on gpmo_cehvi_argbest's first call
template <int NOBJ, int FORM>
static int cehvi_lds_attr_of(gpbo_ctx* ctx) {
  const void* kernels[] = {
      reinterpret_cast<const void*>(cehvi_kernel<256, NOBJ, FORM>), reinterpret_cast<const void*>(cehvi_kernel<128, NOBJ, FORM>),
      reinterpret_cast<const void*>(cehvi_kernel<64, NOBJ, FORM>),  reinterpret_cast<const void*>(cehvi_kernel<32, NOBJ, FORM>)};
  for (const void* k : kernels) GPBO_HIP(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, EHVI_LDS_BYTES));
  return GPBO_OK;
}
static int cehvi_lds_attr(gpbo_ctx* ctx) {
  if (ctx->func_attrs & ATTR_CEHVI) return GPBO_OK;
  int rc;
  if ((rc = cehvi_lds_attr_of<2, EHVI_PRODUCT>(ctx)) || (rc = cehvi_lds_attr_of<2, EHVI_LOG>(ctx)) ||
      (rc = cehvi_lds_attr_of<3, EHVI_PRODUCT>(ctx)) || (rc = cehvi_lds_attr_of<3, EHVI_LOG>(ctx)))
    return rc;
  ctx->func_attrs |= ATTR_CEHVI;
  return GPBO_OK;
}

// the values of both entry points; feas == nullptr: gpbo_ehvi_argbest's
static int ehvi_values(gpbo_ctx* ctx, int n_obj, int64_t M, const int* n_levels, const double* levels, int64_t n_cells,
                       const uint8_t* cell_lo, const uint8_t* cell_hi, const EhviFeas* feas, int log_form) {
  int rc;
  if ((rc = feas ? cehvi_lds_attr(ctx) : ehvi_lds_attr(ctx))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  // the call's workspace: the level rows, then one word per cell
  const int64_t n_lv = (int64_t)n_obj * GPBO_MAX_EHVI_LEVELS;
  if ((rc = ensure(ctx, &ctx->ehvi, &ctx->cap_ehvi, n_lv + n_cells))) return rc;
  std::vector<double> host((size_t)(n_lv + n_cells), 0.0);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(host.data() + n_lv);
  EhviDev a{};
  a.l_max = 0;
  for (int j = 0; j < n_obj; ++j) {
    for (int l = 0; l < n_levels[j]; ++l) host[(size_t)j * GPBO_MAX_EHVI_LEVELS + l] = levels[(size_t)j * GPBO_MAX_EHVI_LEVELS + l];
    a.mu[j] = ctx->models[j].mu; a.sd[j] = ctx->models[j].sd; a.n_levels[j] = n_levels[j];
    if (n_levels[j] > a.l_max) a.l_max = n_levels[j];
  }
  for (int64_t k = 0; k < n_cells; ++k) {
    unsigned long long w = 0;
    for (int j = 0; j < n_obj; ++j)
      w |= (unsigned long long)cell_lo[k * n_obj + j] << (8 * j) | (unsigned long long)cell_hi[k * n_obj + j] << (8 * (3 + j));
    words[k] = w;
  }
  GPBO_HIP(ctx, hipMemcpyAsync(ctx->ehvi, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));      // `host` is pageable and leaves scope
  const int C = ehvi_tile(n_obj * a.l_max), G = EHVI_THREADS / C;
  a.levels = ctx->ehvi;
  a.cells = reinterpret_cast<const unsigned long long*>(ctx->ehvi + n_lv);
  a.n_cells = (int)n_cells;
  a.per_group = (int)((n_cells + G - 1) / G);
  a.M = M;
  const size_t lds = (size_t)n_obj * a.l_max * C * sizeof(double);
  return n_obj == 2 ? ehvi_launch_tile<2>(ctx, a, C, lds, feas, log_form) : ehvi_launch_tile<3>(ctx, a, C, lds, feas, log_form);
}

int launch_ehvi_values(gpbo_ctx* ctx, int n_obj, int64_t M, const int* n_levels, const double* levels, int64_t n_cells,
                       const uint8_t* cell_lo, const uint8_t* cell_hi) {
  return ehvi_values(ctx, n_obj, M, n_levels, levels, n_cells, cell_lo, cell_hi, nullptr, 0);
}

int launch_cehvi_values(gpbo_ctx* ctx, int n_obj, int64_t M, const int* n_levels, const double* levels, int64_t n_cells,
                        const uint8_t* cell_lo, const uint8_t* cell_hi, int n_constraints, const double* lb, const double* ub,
                        int log_form) {
  EhviFeas feas{};
  feas.n = n_constraints;
  for (int j = 0; j < n_constraints; ++j) {
    const Model& m = ctx->models[n_obj + j];
    feas.cm[j] = m.mu; feas.cs[j] = m.sd; feas.lb[j] = lb[j]; feas.ub[j] = ub[j];
  }
  return ehvi_values(ctx, n_obj, M, n_levels, levels, n_cells, cell_lo, cell_hi, &feas, log_form);
}

}  // namespace gpbo

#ifdef GPBO_DEBUG
using namespace gpbo;

extern "C" int gpbo_debug_ehvi_ms(gpbo_ctx* ctx, float* ms) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!ms) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_ehvi_ms: NULL output");
  if (!ctx->ehvi_ev_used) GPBO_FAIL(ctx, GPBO_ERR_STATE, "debug_ehvi_ms: no gpbo_ehvi_argbest call to report");
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  GPBO_HIP(ctx, hipEventElapsedTime(ms, ctx->ehvi_ev[0], ctx->ehvi_ev[1]));
  return GPBO_OK;
}
#endif
