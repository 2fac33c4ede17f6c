// gpbo_generate_candidates_trust_region: the candidate set of a trust-region step (TuRBO; Eriksson et al. 2019) generated in HBM.
// include/gpbo.h has the definition of an element; in short, row m is the centre with a few coordinates replaced by the m-th point
// of a scrambled Sobol sequence mapped into [lo, hi]:
//   Sobol word   w(m, t) = shift[t] ^ XOR_{b set in g} sv[t][b],  g = m ^ (m >> 1);   point = lo[t] + (hi[t] - lo[t]) * (w 2^-bits)
//   mask         element e = m d + t is perturbed iff word (e & 3) of philox4x32_10((e >> 2, 0, 0), key) < threshold
//   fallback     a row without a perturbed coordinate gets column (w0 d) >> 32, w0 = word 0 of philox4x32_10((m, 1, 0), key)
//
// The pass is bound by its stores (8 M d bytes).  A workgroup owns a run of whole consecutive rows that starts on a Philox quad
// (a multiple of four elements), so one Philox call serves four consecutive elements of one thread, the stores are two 16-byte
// stores per thread over one contiguous range per workgroup, and "no coordinate perturbed" is decided inside the workgroup:
//   trust_region_wave_kernel   d = 4, 8, 16, 32, 64: a row is 1 .. 16 aligned lanes of one wave; the test is a ballot
//   trust_region_rows_kernel   every other d (a quad may straddle two rows): mask bits and fallback columns through LDS
// The direction numbers (at most 32 x 64 words, transposed to [bit][column] so that a thread's four columns are one 16-byte LDS
// read) are staged in LDS once per workgroup, only the bits an index below M can have set; a Sobol word is formed only where the
// mask is set, popcount(g) XORs each.  The wave kernel's rows are a power of two and start at a multiple of it, so the high bits of g
// are the workgroup's: their direction numbers are folded into the staged shift once, and a row XORs its low bits only
// (8 at d = 16, 6 at d = 64: 4 and 3 LDS reads on average instead of log2(M) / 2).  No scratch, no atomics, one launch.  (-ffp-contract=off: lo + (hi - lo) * u rounds as NumPy's.)
#include "gpbo_internal.h"
#include "philox.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace gpbo {

constexpr int TR_THREADS = 256;
constexpr int TR_QUADS = 1024;       // Philox quads (four elements each) a workgroup owns at most: 32 KiB of candidates
constexpr int TR_MAX_BITS = 32;
// the call's arguments in ctx->red: centre | lo | hi (GPBO_MAX_DIM doubles each), shift[GPBO_MAX_DIM], sv transposed [bit][GPBO_MAX_DIM]
constexpr size_t TR_OFF_SHIFT = 3 * GPBO_MAX_DIM * sizeof(double);
constexpr size_t TR_OFF_SV = TR_OFF_SHIFT + GPBO_MAX_DIM * sizeof(unsigned);
constexpr size_t TR_ARG_BYTES = TR_OFF_SV + (size_t)TR_MAX_BITS * GPBO_MAX_DIM * sizeof(unsigned);
static_assert(TR_OFF_SHIFT % 16 == 0 && TR_OFF_SV % 16 == 0, "the tables are read 16 bytes at a time");

struct alignas(16) TrTables {
  unsigned sv[TR_MAX_BITS * GPBO_MAX_DIM];   // [bit][column]
  unsigned shift[GPBO_MAX_DIM];
  double box[3 * GPBO_MAX_DIM];              // centre | lo | hi
};

struct TrArgs {
  double* Xc;
  int64_t M;
  int d;
  int n_bits;             // bits an index below M can have set: only those rows of sv are staged
  double scale;           // 2^-bits
  unsigned long long threshold;
  unsigned k0, k1;
  const char* tables;     // the layout above
};

// The workgroup's tables into LDS.  g_fixed: the Gray-code bits every row of the workgroup has in common (bits >= lds_bits only);
// their direction numbers are folded into the staged shift once, so a row XORs only the bits below lds_bits that it has set.
__device__ __forceinline__ void tr_stage(TrTables& s, const TrArgs& a, int lds_bits, unsigned g_fixed) {
  const unsigned* gsv = (const unsigned*)(a.tables + TR_OFF_SV);
  uint4* lsv = (uint4*)s.sv;
  for (int i = threadIdx.x; i < lds_bits * (GPBO_MAX_DIM / 4); i += TR_THREADS) lsv[i] = ((const uint4*)gsv)[i];
  if (threadIdx.x < GPBO_MAX_DIM) {
    unsigned w = ((const unsigned*)(a.tables + TR_OFF_SHIFT))[threadIdx.x];
    for (unsigned g = g_fixed; g; g &= g - 1) w ^= gsv[(__ffs(g) - 1) * GPBO_MAX_DIM + threadIdx.x];
    s.shift[threadIdx.x] = w;
  }
  if (threadIdx.x < 3 * GPBO_MAX_DIM) s.box[threadIdx.x] = ((const double*)a.tables)[threadIdx.x];
  __syncthreads();
}

// the four mask bits of Philox quad q
__device__ __forceinline__ unsigned tr_quad_mask(const TrArgs& a, int64_t q) {
  unsigned c[4] = {(unsigned)q, (unsigned)((unsigned long long)q >> 32), 0u, 0u};
  philox4x32_10(c, a.k0, a.k1);
  unsigned nib = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) nib |= (unsigned)((unsigned long long)c[j] < a.threshold) << j;
  return nib;
}

// the one column row m perturbs when its mask is empty
__device__ __forceinline__ int tr_fallback_column(const TrArgs& a, int64_t m) {
  unsigned c[4] = {(unsigned)m, (unsigned)((unsigned long long)m >> 32), 1u, 0u};
  philox4x32_10(c, a.k0, a.k1);
  return (int)(((unsigned long long)c[0] * (unsigned)a.d) >> 32);
}

__device__ __forceinline__ double tr_point(const TrTables& s, int t, unsigned w, double scale) {
  const double lo = s.box[GPBO_MAX_DIM + t], hi = s.box[2 * GPBO_MAX_DIM + t];
  return lo + (hi - lo) * ((double)w * scale);      // w 2^-bits is exact
}

__device__ __forceinline__ void tr_store4(double* p, const double (&v)[4]) {
  *(double2*)p = make_double2(v[0], v[1]);
  *(double2*)(p + 2) = make_double2(v[2], v[3]);
}

// d = 4 << lc, lc = 0 .. 4: quad q covers columns [4 (q & (cpr - 1)), + 4) of row q >> lc, cpr = 1 << lc lanes per row
__global__ __launch_bounds__(TR_THREADS) void trust_region_wave_kernel(TrArgs a, int lc) {
  __shared__ TrTables s;
  // the workgroup's TR_QUADS >> lc rows start at a multiple of their count: they differ in the low `lr` bits of m only, so bit b >=
  // lr of g = m ^ (m >> 1) is the same for all of them
  constexpr int TR_LOG_QUADS = 10;
  static_assert(TR_QUADS == 1 << TR_LOG_QUADS, "a workgroup's rows are a power of two");
  const int lr = TR_LOG_QUADS - lc;
  const unsigned m0 = (unsigned)(((int64_t)blockIdx.x * TR_QUADS) >> lc);
  const unsigned low = (1u << lr) - 1u;
  tr_stage(s, a, a.n_bits < lr ? a.n_bits : lr, (m0 ^ (m0 >> 1)) & ~low);
  const int cpr = 1 << lc;
  const int64_t nq = a.M << lc;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < TR_QUADS / TR_THREADS; ++k) {        // a counted loop: every lane reaches the ballot
    const int64_t q = (int64_t)blockIdx.x * TR_QUADS + k * TR_THREADS + threadIdx.x;
    const int64_t m = q >> lc;
    const int part = (int)(q & (cpr - 1));
    unsigned nib = tr_quad_mask(a, q);
    const unsigned long long any = __ballot(nib != 0);
    if ((unsigned)(any >> (lane & ~(cpr - 1))) << (32 - cpr) == 0u) {      // none of the row's cpr lanes has a bit (the row's lanes agree)
      const int col = tr_fallback_column(a, m);
      if ((col >> 2) == part) nib = 1u << (col & 3);
    }
    if (q >= nq) continue;       // (rows are whole: a row's lanes leave together)
    const int t0 = 4 * part;
    double v[4] = {s.box[t0], s.box[t0 + 1], s.box[t0 + 2], s.box[t0 + 3]};
    if (nib) {
      uint4 w = *(const uint4*)&s.shift[t0];
      for (unsigned g = ((unsigned)m ^ ((unsigned)m >> 1)) & low; g; g &= g - 1) {
        const uint4 x = *(const uint4*)&s.sv[(__ffs(g) - 1) * GPBO_MAX_DIM + t0];
        w.x ^= x.x; w.y ^= x.y; w.z ^= x.z; w.w ^= x.w;
      }
      if (nib & 1u) v[0] = tr_point(s, t0, w.x, a.scale);
      if (nib & 2u) v[1] = tr_point(s, t0 + 1, w.y, a.scale);
      if (nib & 4u) v[2] = tr_point(s, t0 + 2, w.z, a.scale);
      if (nib & 8u) v[3] = tr_point(s, t0 + 3, w.w, a.scale);
    }
    tr_store4(a.Xc + 4 * q, v);
  }
}

// any d: the workgroup owns `rows` rows (a multiple of 4, rows * d <= 4 TR_QUADS), its elements start on a quad
__global__ __launch_bounds__(TR_THREADS) void trust_region_rows_kernel(TrArgs a, int rows) {
  __shared__ TrTables s;
  __shared__ unsigned char mask[TR_QUADS];        // a quad's four mask bits
  __shared__ unsigned char fallback[4 * TR_QUADS];   // a row's fallback column; 0xFF: the row has a perturbed coordinate
  tr_stage(s, a, a.n_bits, 0u);
  const int d = a.d;
  const int64_t r0 = (int64_t)blockIdx.x * rows;
  const int nr = (int)(a.M - r0 < rows ? a.M - r0 : rows);
  const int ne = nr * d;
  const int nq = (ne + 3) >> 2;
  const int64_t q0 = (r0 * d) >> 2;
  for (int qi = threadIdx.x; qi < nq; qi += TR_THREADS) mask[qi] = (unsigned char)tr_quad_mask(a, q0 + qi);
  __syncthreads();
  for (int r = threadIdx.x; r < nr; r += TR_THREADS) {
    unsigned any = 0;
    for (int e = r * d; e < (r + 1) * d; ++e) any |= (mask[e >> 2] >> (e & 3)) & 1u;
    fallback[r] = any ? (unsigned char)0xFF : (unsigned char)tr_fallback_column(a, r0 + r);
  }
  __syncthreads();
  for (int qi = threadIdx.x; qi < nq; qi += TR_THREADS) {
    const unsigned nib = mask[qi];
    const int e0 = 4 * qi;
    int r = e0 / d, t = e0 - r * d;
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = 0.0;
      if (e0 + j < ne) {
        v[j] = s.box[t];
        if (((nib >> j) & 1u) || fallback[r] == t) {
          unsigned w = s.shift[t];
          const unsigned m = (unsigned)(r0 + r);
          for (unsigned g = m ^ (m >> 1); g; g &= g - 1) w ^= s.sv[(__ffs(g) - 1) * GPBO_MAX_DIM + t];
          v[j] = tr_point(s, t, w, a.scale);
        }
        if (++t == d) { t = 0; ++r; }
      }
    }
    double* p = a.Xc + r0 * d + e0;
    if (e0 + 3 < ne) {
      tr_store4(p, v);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < ne) p[j] = v[j];
    }
  }
}

// debug build: an event before and after the generator kernel of the last gpbo_generate_candidates / _trust_region call
// (gpbo_debug_generate_ms); the product records nothing
void generate_mark(gpbo_ctx* ctx, int i) {
#ifdef GPBO_DEBUG
  if (!ctx->gen_ev[i]) (void)hipEventCreate(&ctx->gen_ev[i]);
  (void)hipEventRecord(ctx->gen_ev[i], ctx->stream);
  ctx->gen_ev_used = (i == 1);
#else
  (void)ctx; (void)i;
#endif
}

}  // namespace gpbo

using namespace gpbo;

extern "C" int gpbo_generate_candidates_trust_region(gpbo_ctx* ctx, int64_t M, int d, const double* centre, const double* lo,
                                                     const double* hi, const uint32_t* sobol_sv, int bits,
                                                     const uint32_t* sobol_shift, uint64_t mask_threshold, uint64_t mask_key) {
  if (!ctx) return GPBO_ERR_INVALID;
  // every refusal comes before the first write: the resident candidates stay as they were
  if (!centre || !lo || !hi || !sobol_sv || !sobol_shift)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "generate_candidates_trust_region: NULL argument");
  if (M < 1) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "generate_candidates_trust_region: M must be >= 1");
  if (d < 1 || d > GPBO_MAX_DIM) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "generate_candidates_trust_region: d out of range [1, 64]");
  if (bits < 1 || bits > TR_MAX_BITS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "generate_candidates_trust_region: bits out of range [1, 32]");
  if (M > ((int64_t)1 << bits))
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "generate_candidates_trust_region: M exceeds the 2^bits points of the sequence");
  if (mask_threshold > ((uint64_t)1 << 32))
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "generate_candidates_trust_region: mask_threshold exceeds 2^32");
  for (int t = 0; t < d; ++t) {
    if (!std::isfinite(centre[t]) || !std::isfinite(lo[t]) || !std::isfinite(hi[t]))
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, "generate_candidates_trust_region: centre, lo and hi must be finite");
    if (lo[t] > hi[t]) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "generate_candidates_trust_region: lo exceeds hi");
  }
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure(ctx, &ctx->Xc, &ctx->cap_Xc, M * d))) return rc;
  {
    char* p = (char*)ctx->red;
    int64_t cap = ctx->cap_red;
    if ((rc = ensure(ctx, &p, &cap, (int64_t)TR_ARG_BYTES + 4096))) return rc;
    ctx->red = p;
    ctx->cap_red = cap;
  }
  // from here on the buffer belongs to the new matrix
  ctx->raw_valid = false;
  ctx->M = M;
  ctx->d_c = d;
  drop_posteriors(ctx);

  TrArgs a;
  a.Xc = ctx->Xc;
  a.M = M;
  a.d = d;
  a.n_bits = 0;
  while (a.n_bits < bits && ((int64_t)1 << a.n_bits) < M) ++a.n_bits;       // g = m ^ (m >> 1) is as long as m <= M - 1
  a.scale = std::ldexp(1.0, -bits);
  a.threshold = mask_threshold;
  a.k0 = (unsigned)mask_key;
  a.k1 = (unsigned)(mask_key >> 32);
  a.tables = (const char*)ctx->red;

  std::vector<char> host(TR_ARG_BYTES, 0);      // (alive until the stream is synchronised below)
  double* box = (double*)host.data();
  unsigned* shift = (unsigned*)(host.data() + TR_OFF_SHIFT);
  unsigned* sv = (unsigned*)(host.data() + TR_OFF_SV);
  for (int t = 0; t < d; ++t) {
    box[t] = centre[t];
    box[GPBO_MAX_DIM + t] = lo[t];
    box[2 * GPBO_MAX_DIM + t] = hi[t];
    shift[t] = sobol_shift[t];
    for (int b = 0; b < a.n_bits; ++b) sv[b * GPBO_MAX_DIM + t] = sobol_sv[(size_t)t * bits + b];
  }
  hipError_t e = hipMemcpyAsync(ctx->red, host.data(), TR_ARG_BYTES, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    generate_mark(ctx, 0);
    int lc = -1;
    for (int k = 0; k <= 4; ++k)
      if (d == (4 << k)) lc = k;
    if (lc >= 0) {
      const int64_t blocks = ((M << lc) + TR_QUADS - 1) / TR_QUADS;
      trust_region_wave_kernel<<<dim3((unsigned)blocks), dim3(TR_THREADS), 0, ctx->stream>>>(a, lc);
    } else {
      const int rows = (4 * TR_QUADS / d) & ~3;       // >= 64 for d <= 63
      const int64_t blocks = (M + rows - 1) / rows;
      trust_region_rows_kernel<<<dim3((unsigned)blocks), dim3(TR_THREADS), 0, ctx->stream>>>(a, rows);
    }
    e = hipGetLastError();
    generate_mark(ctx, 1);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  GPBO_HIP(ctx, e);
  GPBO_HIP(ctx, es);
  return GPBO_OK;
}

#ifdef GPBO_DEBUG
extern "C" int gpbo_debug_generate_ms(gpbo_ctx* ctx, float* ms) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!ms) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_generate_ms: NULL output");
  if (!ctx->gen_ev_used) GPBO_FAIL(ctx, GPBO_ERR_STATE, "debug_generate_ms: no generator call to report");
  GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  GPBO_HIP(ctx, hipEventElapsedTime(ms, ctx->gen_ev[0], ctx->gen_ev[1]));
  return GPBO_OK;
}
#endif
