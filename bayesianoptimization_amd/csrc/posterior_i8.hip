// posterior_i8 — the posterior's triangular GEMM V = W K*^T and sum_i v_i^2 on the int8 matrix cores, exact to fp64
// accuracy (fixed-point Ozaki scheme: i8_digits.h).
//
// Why: the fp64 slab GEMM (posterior_kernel_v2.hip, GEN = 2) runs at 0.93 of the fp64 matrix peak and is 92 % of a C3
// step.  v_mfma_i32_16x16x64_i8 does 16 384 MACs in half the cycles v_mfma_f64_16x16x4_f64 takes for 512: with both operands
// split into I8_S = 7 int8 digit planes, the 28 products (s, t), s + t <= S - 1, cost less than half the fp64 GEMM's
// matrix-pipe time, and integer sums are exact.
//
//   workgroup = 4 waves (one per SIMD), 128 rows of W x 64 candidates; heaviest row chunks first, as in v2;
//   wave w    = two 16-row blocks x four 16-candidate blocks = 8 x S int32 accumulator tiles (224 registers);
//   k step    = 64 train points: 2 S A fragments (the wave's rows) + 4 S B fragments (k* digits), 16 B per lane each, in
//               fragment order (i8_frag_index); each fragment feeds up to 4 S products, 224 per step;
//   triangle  = a wave walks the k steps 0 ... the one that holds its own diagonal only (the digit planes of W are packed as
//               the lower triangle, zero past the diagonal inside the last step).
// The MFMA shape: 16x16x64 and 32x32x32 do the same MACs per cycle; the tile per wave, the bytes per k and the summation order
// of the epilogue are those of the 32x32x32 kernel this one replaced, so the results are the same bits.
// The operand lane maps of the int8 MFMA need not be known: A and B use the same (lane group, byte) -> k assignment, and the
// sum over k does not care which k sits where.  The C/D map (col = lane & 15, row = 4 (lane >> 4) + reg, the same for every
// non-f64 16 x 16 MFMA on gfx950) places each row's scale and each candidate's sum.
//
// The level sums are exact, so v_i is the correctly rounded value of the truncated digit product whatever the tiling; the
// sum of squares is then taken in a fixed order per 128-row chunk, as the fp64 kernels do per 256-row chunk.  mu (k* . alpha)
// is computed by kstar_gen_kernel exactly as on the fp64 path.
#include <algorithm>

#include "gpbo_internal.h"
#include "i8_digits.h"
#include "posterior_tile.h"

namespace gpbo {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int I8_CANDS = 64;   // candidates per workgroup (4 blocks of 16)

// ---- W -> digit planes, once per fit ----------------------------------------------------------------------------------
// Row exponents: one wave per row, max |W_ij| over the row's N x N lower-triangle part (order-free, so deterministic).
__global__ __launch_bounds__(256) void wd_row_scale_kernel(const double* __restrict__ W, int* __restrict__ wexp,
                                                           double* __restrict__ wscale, int64_t N, int64_t NP) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= NP) return;
  double mx = 0.0;
  if (row < N)
    for (int64_t j = lane; j <= row; j += 64) mx = fmax(mx, fabs(W[row * NP + j]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  if (lane == 0) {
    const int e = i8_row_exponent(mx);
    wexp[row] = e;
    wscale[row] = ldexp(1.0, i8_scale_exp<I8_S>(e));
  }
}

// Digit planes: thread = (16-row block b, 64-step ks <= b / 4, lane); lane 16 g + r holds row 16 b + r, columns 64 ks + 16 g + j.
// Layout: i8_frag_index from the block's first step i8_wd_block(b).  Entries outside the N x N lower triangle are zero (as
// pack_w_elem), the part of a block's last step past its diagonal included.
__global__ __launch_bounds__(256) void wd_pack_kernel(const double* __restrict__ W, const int* __restrict__ wexp,
                                                      uint4* __restrict__ Wd, int64_t N, int64_t NP) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int ks = t >> 6, lane = t & 63;
  if (ks > b / 4) return;
  const int64_t row = (int64_t)b * 16 + (lane & 15);
  const int64_t c0 = (int64_t)ks * 64 + (lane >> 4) * 16;
  const int e = wexp[row];
  uint32_t w[I8_S][4] = {};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int64_t col = c0 + j;
    const double x = (row < N && col < N && col <= row) ? W[row * NP + col] : 0.0;
    const int64_t q = i8_quantize<I8_S>(ldexp(x, -e));
#pragma unroll
    for (int s = 0; s < I8_S; ++s) w[s][j >> 2] |= i8_digit_byte<I8_S>(q, s) << (8 * (j & 3));
  }
  uint4* dst = Wd + i8_frag_index<I8_S>(i8_wd_block(b), c0, 0, lane & 15);
#pragma unroll
  for (int s = 0; s < I8_S; ++s) dst[s * 64] = make_uint4(w[s][0], w[s][1], w[s][2], w[s][3]);
}

static int pack_wd(gpbo_ctx* ctx, Model& m) {
  const int64_t nb = m.NP / 16;   // NP is a multiple of 64 (prepare_posterior_i8)
  int rc;
  if ((rc = ensure(ctx, &m.Wd, &m.cap_Wd, i8_wd_block(nb) * I8_S * 64))) return rc;
  if ((rc = ensure(ctx, &m.wscale, &m.cap_wscale, 2 * m.NP))) return rc;
  int* wexp = reinterpret_cast<int*>(m.wscale + m.NP);   // the row exponents behind the scales
  wd_row_scale_kernel<<<dim3((unsigned)((m.NP + 3) / 4)), dim3(256), 0, ctx->stream>>>(m.W, wexp, m.wscale, m.N, m.NP);
  GPBO_HIP(ctx, hipGetLastError());
  wd_pack_kernel<<<dim3((unsigned)((m.NP + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream>>>(m.W, wexp, m.Wd, m.N, m.NP);
  GPBO_HIP(ctx, hipGetLastError());
  m.wd_valid = true;
  return GPBO_OK;
}

// ---- the GEMM ---------------------------------------------------------------------------------------------------------
struct I8Args {
  const uint4* Wd;
  const double* wscale;
  const uint4* Kd;     // the slab's digit planes (kstar_gen_kernel<.., SlabI8>)
  double* part;        // [chunk of 128 rows][Mp] sums of squares
  PostGrid g;          // 128-row chunks x 64-candidate tiles of the slab
  int64_t m0;          // first candidate of the slab
};

template <int S>
__global__ __launch_bounds__(256, 1) void posterior_i8_kernel(I8Args p) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  int r, ct;
  p.g.map(blockIdx.x, r, ct);
  const int nks = p.g.NP / 64;
  const int rb = r * (I8_ROWS / 32) + wave;     // this wave's 32 rows: the 16-row blocks 2 rb and 2 rb + 1
  const bool active = rb < p.g.NP / 32;           // false only in a ragged last chunk

  __shared__ double red[4][I8_CANDS];
  double ss[4] = {0.0, 0.0, 0.0, 0.0};   // per candidate block: sum of v^2 over the wave's rows (see the epilogue)
  if (active) {
    v4i acc[2][4][S];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int l = 0; l < S; ++l) acc[a][j][l] = v4i{};
    // Operands through buffer descriptors (wave-uniform bases, the lane as a constant 32-bit offset, the block and the walk along k
    // as the scalar offset), as in posterior_kernel_v2: no 64-bit address arithmetic per load.
    const int n = rb / 2 + 1;                   // 64-steps up to the diagonal: both 16-row blocks hold exactly these
    const uint4* wa = p.Wd + i8_wd_block(2 * rb) * S * 64;
    const uint4* kb0 = p.Kd + i8_kd_block(4 * ct, p.g.NP) * S * 64;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(wa), 0, 0x7fffffff, BUF_FLAGS);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(kb0), 0, 0x7fffffff, BUF_FLAGS);
    const unsigned voff = (unsigned)lane * 16u;
    const unsigned sofA = (unsigned)n * S * 1024u, sofB = (unsigned)nks * S * 1024u;   // block strides, scalar like the k walk
    // One operand set is 6 S fragments = 168 registers, so beside 224 accumulators there is ONE set, and each part of it is
    // re-loaded for the next step as soon as its last product of this step has issued.  A step is four phases of 2 S (S + 1)
    // = 56 products: A0 x B01, A1 x B01, A0 x B23, A1 x B23 (A0 / A1 the upper / lower 16 rows, B01 / B23 the candidate blocks 0, 1
    // / 2, 3).  B01 is free after the second phase, A0 after the third, A1 and B23 after the fourth: k* digits (which come from
    // beyond L2) are in flight for two phases before their first use, W digits (L2) for one.
    v4i a[2][S], b[4][S];
    auto load_a = [&](int ks, int i) {
      const unsigned o = (unsigned)ks * S * 1024u + i * sofA;
#pragma unroll
      for (int s = 0; s < S; ++s)
        a[i][s] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(rsA, voff, o + s * 1024u, 0));
    };
    auto load_b = [&](int ks, int j0) {
      const unsigned o = (unsigned)ks * S * 1024u;
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int j = j0; j < j0 + 2; ++j)
          b[j][s] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(rsB, voff, o + j * sofB + s * 1024u, 0));
    };
    // (s, t) with s + t <= S - 1, level l = s + t; consecutive products go to different accumulators
    auto mma = [&](int i, int j0) {
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int t = 0; t + s < S; ++t)
#pragma unroll
          for (int j = j0; j < j0 + 2; ++j)
            acc[i][j][s + t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i][s], b[j][t], acc[i][j][s + t], 0, 0, 0);
    };
    // (the first step's loads in the order of their use, as every later step's: the wait counts of the loop body are those of
    // the worse of its two entries)
    load_a(0, 0);
    load_b(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    load_a(0, 1);
    __builtin_amdgcn_sched_barrier(0);
    load_b(0, 2);
#pragma unroll 1
    for (int ks = 0; ks < n; ++ks) {
      // the look-ahead past the last step reloads the last step (in bounds, unused): the body has no branch.
      // sched_barrier: hipcc otherwise sinks the loads next to their first use
      const int nx = min(ks + 1, n - 1);
      __builtin_amdgcn_sched_barrier(0);
      mma(0, 0);
      __builtin_amdgcn_sched_barrier(0);   // (A1 and B23, loaded last, are still in flight here)
      mma(1, 0);
      __builtin_amdgcn_sched_barrier(0);
      load_b(nx, 0);
      __builtin_amdgcn_sched_barrier(0);
      mma(0, 2);
      __builtin_amdgcn_sched_barrier(0);
      load_a(nx, 0);
      __builtin_amdgcn_sched_barrier(0);
      mma(1, 2);
      __builtin_amdgcn_sched_barrier(0);
      load_a(nx, 1);
      load_b(nx, 2);
    }

    // epilogue: v = (exact level sum, rounded once) x 2^(row scale); sum of v^2 over the wave's rows.  The order is the one of the
    // 32 x 32 C layout, whose lane half h held rows 4 h + {0-3, 8-11, 16-19, 24-27} as ONE fma chain: here lane group g = lane >> 4
    // holds rows 4 g + reg of the upper (a = 0) and lower (a = 1) 16-row tile, so the chain of half h runs through group h (rows
    // 4 h + 0-3), group h + 2 (+ 8), group h (+ 16), group h + 2 (+ 24), handed over by three cross-lane moves.  Every lane runs
    // both legs of a tile; the leg that does not belong to its group computes a value nobody reads.
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        double v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = rb * 32 + 16 * a + 4 * (lane >> 4) + i;
          int32_t lv[S];
#pragma unroll
          for (int l = 0; l < S; ++l) lv[l] = acc[a][j][l][i];
          v[i] = i8_combine<S>(lv) * p.wscale[row];
          __builtin_amdgcn_sched_barrier(0);   // one output at a time: hoisting all 224 accumulator reads spills
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) s = fma(v[i], v[i], s);   // groups 0, 1: their rows of this tile
        s = __shfl_xor(s, 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) s = fma(v[i], v[i], s);   // groups 2, 3: theirs, on top
        if (a == 0) s = __shfl_xor(s, 32);
      }
      ss[j] = s;   // groups 2, 3: the chain of half 0, of half 1
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double o = __shfl_xor(ss[j], 16);
    if ((lane >> 4) == 2) red[wave][j * 16 + (lane & 15)] = ss[j] + o;   // half 0's sum + half 1's
  }
  __syncthreads();
  if (tid < I8_CANDS) {
    const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    p.part[(int64_t)r * p.g.Mp + p.m0 + (int64_t)ct * I8_CANDS + tid] = v;
  }
}

// ---- dispatch ---------------------------------------------------------------------------------------------------------
// SlabI8 (posterior_plan.h) in the slab walk (launch_posterior_slabs): the slab is I8_S bytes per element and its width comes from
// i8_slab_width: small enough that the 32 row chunks re-read it from the 256 MB Infinity Cache rather than from HBM, and such that
// the generation's grid ends with the device's compute units full (GPBO_KSTAR_GB still caps it).  The byte bound I8_SLAB_BYTES is
// a constant of the rule: the debug build's slab-size switch (GPBO_I8_SLAB_MB, which produced the table quoted there) went with
// the plain byte rule, so another bound is probed by rebuilding.
// One slab's launch: a workgroup per (128-row chunk, 64-candidate tile of the slab), the chunk outermost (heaviest first).  `part`
// is [nchunks][Mp]; the slab holds the candidates m0 ... m0 + ldk (ldk a multiple of 64).
static int launch_i8_gemm(gpbo_ctx* ctx, const uint4* Wd, const double* wscale, const uint4* Kd, double* part, int64_t NP, int64_t Mp,
                          int nchunks, int64_t ldk, int64_t m0) {
  I8Args a;
  a.Wd = Wd; a.wscale = wscale; a.Kd = Kd; a.part = part;
  a.g = {(int)NP, Mp, nchunks, (int)(ldk / I8_CANDS)};
  a.m0 = m0;
  posterior_i8_kernel<I8_S><<<dim3((unsigned)a.g.blocks()), dim3(256), 0, ctx->stream>>>(a);
  GPBO_HIP(ctx, hipGetLastError());
  return GPBO_OK;
}

// ... with the model's own digit planes of W, for one slab of the walk
int launch_slab_gemm_i8(gpbo_ctx* ctx, Model& m, const void* slab, int64_t ldk, int64_t m0, int64_t Mp, int part_chunks) {
  return launch_i8_gemm(ctx, m.Wd, m.wscale, static_cast<const uint4*>(slab), ctx->part, m.NP, Mp, part_chunks, ldk, m0);
}

// What the walk needs before its first int8 slab: the size check, W's digit planes (once per fit) and the device's compute units
// (once per context: i8_slab_width fills them).
int prepare_posterior_i8(gpbo_ctx* ctx, Model& m) {
  if (m.NP > I8_NP_MAX || m.NP % 64) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "posterior: the int8 GEMM serves NP <= 16384");
  int rc;
  if (!m.wd_valid && (rc = pack_wd(ctx, m))) return rc;
  if (!ctx->compute_units) GPBO_HIP(ctx, hipDeviceGetAttribute(&ctx->compute_units, hipDeviceAttributeMultiprocessorCount, ctx->device));
  return GPBO_OK;
}

}  // namespace gpbo

#ifdef GPBO_DEBUG   // the stages of the int8 pass alone (include/gpbo.h, "debug build"): tests/test_gpu_int8_exact.py
using namespace gpbo;

static bool i8_debug_np_ok(int64_t NP) { return NP >= 64 && NP <= I8_NP_MAX && NP % 64 == 0; }

int gpbo_debug_i8_pack_w(gpbo_ctx* ctx, const double* W, int64_t N, int64_t NP, void* Wd_out, int* wexp_out, double* wscale_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!W || !Wd_out || !wexp_out || !wscale_out || !i8_debug_np_ok(NP) || N < 1 || N > NP)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_i8_pack_w: bad arguments (NP a multiple of 64 in [64, 16384], 1 <= N <= NP)");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  Model m;   // a scratch model that owns W, Wd and wscale only: no slot of the context is touched
  m.N = N; m.NP = NP;
  auto done = [&](int code) {
    if (m.W) (void)hipFree(m.W);
    if (m.Wd) (void)hipFree(m.Wd);
    if (m.wscale) (void)hipFree(m.wscale);
    return code;
  };
  const size_t sq = (size_t)NP * NP * sizeof(double);
  if (hipMalloc((void**)&m.W, sq) != hipSuccess) return done(GPBO_ERR_HIP);
  if (hipMemcpy(m.W, W, sq, hipMemcpyHostToDevice) != hipSuccess) return done(GPBO_ERR_HIP);
  int rc = pack_wd(ctx, m);
  if (rc) return done(rc);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return done(GPBO_ERR_HIP);
  const size_t wd_bytes = (size_t)i8_wd_block(NP / 16) * I8_S * 64 * sizeof(uint4);
  if (hipMemcpy(Wd_out, m.Wd, wd_bytes, hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  if (hipMemcpy(wscale_out, m.wscale, (size_t)NP * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  if (hipMemcpy(wexp_out, m.wscale + NP, (size_t)NP * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  return done(GPBO_OK);
}

int gpbo_debug_i8_gemm(gpbo_ctx* ctx, const void* Wd, const double* wscale, const void* Kd, int64_t NP, int64_t M, double* part_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!Wd || !wscale || !Kd || !part_out || !i8_debug_np_ok(NP) || M < I8_CANDS || M % I8_CANDS || M > (1 << 20))
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_i8_gemm: bad arguments (NP a multiple of 64 in [64, 16384], M a multiple of 64)");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  const int nchunks = (int)((NP + I8_ROWS - 1) / I8_ROWS);
  const size_t wd_bytes = (size_t)i8_wd_block(NP / 16) * I8_S * 64 * sizeof(uint4);
  const size_t kd_bytes = (size_t)M * NP * I8_S;
  const size_t part_bytes = (size_t)nchunks * M * sizeof(double);
  uint4 *dW = nullptr, *dK = nullptr;
  double *dS = nullptr, *dP = nullptr;
  auto done = [&](int code) {
    if (dW) (void)hipFree(dW);
    if (dK) (void)hipFree(dK);
    if (dS) (void)hipFree(dS);
    if (dP) (void)hipFree(dP);
    return code;
  };
  if (hipMalloc((void**)&dW, wd_bytes) != hipSuccess || hipMalloc((void**)&dK, kd_bytes) != hipSuccess ||
      hipMalloc((void**)&dS, (size_t)NP * sizeof(double)) != hipSuccess || hipMalloc((void**)&dP, part_bytes) != hipSuccess)
    return done(GPBO_ERR_HIP);
  if (hipMemcpy(dW, Wd, wd_bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dK, Kd, kd_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dS, wscale, (size_t)NP * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dP, 0xff, part_bytes) != hipSuccess)   // NaN where the kernel writes nothing
    return done(GPBO_ERR_HIP);
  const int rc = launch_i8_gemm(ctx, dW, dS, dK, dP, NP, M, nchunks, M, 0);
  if (rc) return done(rc);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return done(GPBO_ERR_HIP);
  if (hipMemcpy(part_out, dP, part_bytes, hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  return done(GPBO_OK);
}
#endif  // GPBO_DEBUG
