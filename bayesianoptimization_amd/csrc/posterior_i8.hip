// posterior_i8 — the posterior's triangular GEMM V = W K*^T and sum_i v_i^2 on the int8 matrix cores, exact to fp64
// accuracy (fixed-point Ozaki scheme: i8_digits.h).
//
// Why: the fp64 slab GEMM (posterior_kernel_v2.hip, GEN = 2) runs at 0.93 of the fp64 matrix peak and is 92 % of a C3
// step.  v_mfma_i32_32x32x32_i8 does 32 768 MACs in the cycles v_mfma_f64_16x16x4_f64 takes for 512: with both operands
// split into I8_S = 7 int8 digit planes, the 28 products (s, t), s + t <= S - 1, cost less than half the fp64 GEMM's
// matrix-pipe time, and integer sums are exact.
//
//   workgroup = 4 waves (one per SIMD), 128 rows of W x 64 candidates; heaviest row chunks first, as in v2;
//   wave w    = one 32-row block x two 32-candidate blocks = 2 x S int32 accumulator tiles (224 registers);
//   k step    = 32 train points: S A fragments (the wave's rows) + 2 S B fragments (k* digits), 16 B per lane each,
//               loaded from memory in fragment order one step ahead; each fragment feeds up to S products.
//   triangle  = a wave walks the k steps 0 ... its own row block only (the digit planes of W are packed as the lower
//               triangle of 32 x 32 blocks, upper parts of the diagonal block zero).
// The operand lane maps of the int8 MFMA need not be known: A and B use the same (lane half, byte) -> k assignment, and the
// sum over k does not care which k sits where.  The C/D map (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5),
// the same for every non-f64 MFMA on gfx950) places each row's scale and each candidate's sum.
//
// The level sums are exact, so v_i is the correctly rounded value of the truncated digit product whatever the tiling; the
// sum of squares is then taken in a fixed order per 128-row chunk, as the fp64 kernels do per 256-row chunk.  mu (k* . alpha)
// is computed by kstar_gen_kernel exactly as on the fp64 path.
#include <algorithm>

#include "gpbo_internal.h"
#include "i8_digits.h"

namespace gpbo {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int I8_CANDS = 64;   // candidates per workgroup (2 blocks of 32)
constexpr int I8_BUF_FLAGS = 0x00020000;   // gfx9 buffer descriptor word 3: raw buffer, 32-bit data format

// first 32 x 32 step of row block rb in the packed W: row blocks 0 ... rb - 1 hold q + 2 steps each
__host__ __device__ inline int64_t wd_block(int64_t rb) { return rb * (rb + 3) / 2; }

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

// Digit planes: thread = (32 x 32 block (rb, ks <= rb + 1), lane); lane 32 h + c holds row 32 rb + c, columns 32 ks + 16 h + j.
// Layout [wd_block(rb) + ks][plane][lane] 16 B.  Entries outside the N x N lower triangle are zero (as pack_w_elem); each row
// block carries one zero step past its diagonal, so that a wave can always walk an even number of steps (see the GEMM).
__global__ __launch_bounds__(256) void wd_pack_kernel(const double* __restrict__ W, const int* __restrict__ wexp,
                                                      uint4* __restrict__ Wd, int64_t N, int64_t NP) {
  const int rb = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int ks = t >> 6, lane = t & 63;
  if (ks > rb + 1) return;
  const int64_t row = (int64_t)rb * 32 + (lane & 31);
  const int64_t c0 = (int64_t)ks * 32 + (lane >> 5) * 16;
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
  uint4* dst = Wd + ((wd_block(rb) + ks) * I8_S) * 64 + lane;
#pragma unroll
  for (int s = 0; s < I8_S; ++s) dst[s * 64] = make_uint4(w[s][0], w[s][1], w[s][2], w[s][3]);
}

static int pack_wd(gpbo_ctx* ctx, Model& m) {
  const int64_t nrb = m.NP / 32;
  int rc;
  if ((rc = ensure(ctx, &m.Wd, &m.cap_Wd, wd_block(nrb) * I8_S * 64))) return rc;
  if ((rc = ensure(ctx, &m.wscale, &m.cap_wscale, 2 * m.NP))) return rc;
  int* wexp = reinterpret_cast<int*>(m.wscale + m.NP);   // the row exponents behind the scales
  wd_row_scale_kernel<<<dim3((unsigned)((m.NP + 3) / 4)), dim3(256), 0, ctx->stream>>>(m.W, wexp, m.wscale, m.N, m.NP);
  GPBO_HIP(ctx, hipGetLastError());
  wd_pack_kernel<<<dim3((unsigned)(((nrb + 1) * 64 + 255) / 256), (unsigned)nrb), dim3(256), 0, ctx->stream>>>(m.W, wexp, m.Wd, m.N,
                                                                                                           m.NP);
  GPBO_HIP(ctx, hipGetLastError());
  m.wd_valid = true;
  return GPBO_OK;
}

// ---- the GEMM ---------------------------------------------------------------------------------------------------------
struct I8Args {
  const uint4* Wd;
  const double* wscale;
  const uint4* Kd;     // the slab's digit planes (kstar_gen_kernel<.., DIG = I8_S>)
  double* part;        // [chunk of 128 rows][Mp] sums of squares
  int NP;
  int64_t Mp;
  int nchunks;         // 128-row chunks
  int n_ctiles;        // 64-candidate tiles of the slab
  int64_t m0;          // first candidate of the slab
};

template <int S>
__global__ __launch_bounds__(256, 1) void posterior_i8_kernel(I8Args p) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int bid = blockIdx.x;
  // Heaviest row chunks first; the workgroups resident at any time share a chunk, so its digit planes of W come out of L2.
  // (Candidate tile outermost instead, so that the row chunks of a tile share its k* digits in L2: 283 ms per C3 pass against 196,
  // with 256 MB ... 4 GB slabs alike.)
  const int r = p.nchunks - 1 - bid / p.n_ctiles;
  const int ct = bid - (bid / p.n_ctiles) * p.n_ctiles;
  const int nks = p.NP / 32;
  const int rb = r * (I8_ROWS / 32) + wave;     // this wave's 32-row block
  const bool active = rb < nks;                 // false only in a ragged last chunk

  __shared__ double red[4][I8_CANDS];
  double ss[2] = {0.0, 0.0};   // per candidate: sum of v^2 over this lane's rows
  if (active) {
    v16i acc[2][S];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int l = 0; l < S; ++l) acc[c][l] = v16i{};
    // Operands through buffer descriptors (wave-uniform bases, the lane as a constant 32-bit offset, the walk along k as the
    // scalar offset), as in posterior_kernel_v2: no 64-bit address arithmetic per load.
    const uint4* wa = p.Wd + wd_block(rb) * S * 64;
    const uint4* kb0 = p.Kd + ((int64_t)(2 * ct) * nks) * S * 64;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(wa), 0, 0x7fffffff, I8_BUF_FLAGS);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(kb0), 0, 0x7fffffff, I8_BUF_FLAGS);
    const unsigned voff = (unsigned)lane * 16u, vofB1 = voff + (unsigned)nks * S * 1024u;
    v4i a[S], b0[S], b1[S], na[S], nb0[S], nb1[S];
    auto load = [&](int ks, v4i(&ra)[S], v4i(&rb0)[S], v4i(&rb1)[S]) {
      const unsigned o = (unsigned)ks * S * 1024u;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        ra[s] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(rsA, voff, o + s * 1024u, 0));
        rb0[s] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(rsB, voff, o + s * 1024u, 0));
        rb1[s] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(rsB, vofB1, o + s * 1024u, 0));
      }
    };
    // (s, t) with s + t <= S - 1, level l = s + t; consecutive products go to different accumulators
    auto mma = [&](const v4i(&ra)[S], const v4i(&rb0)[S], const v4i(&rb1)[S]) {
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int t = 0; t + s < S; ++t) {
          acc[0][s + t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ra[s], rb0[t], acc[0][s + t], 0, 0, 0);
          acc[1][s + t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ra[s], rb1[t], acc[1][s + t], 0, 0, 0);
        }
    };
    // Two register sets, one step of look-ahead each and no copies (a copy waits for its load at once).  The wave walks an
    // even number of steps, rb + 1 or rb + 2: the extra one is the zero step packed past the diagonal (k* exists there:
    // rb even < nks - 1).  The last look-ahead reloads the last step (in bounds, unused): the body has no branch.
    const int n = (rb | 1) + 1;
    load(0, a, b0, b1);
#pragma unroll 1
    for (int ks = 0; ks < n; ks += 2) {
      load(ks + 1, na, nb0, nb1);
      __builtin_amdgcn_sched_barrier(0);   // keep the loads here: hipcc otherwise sinks them next to their first use
      mma(a, b0, b1);
      load(min(ks + 2, n - 1), a, b0, b1);
      __builtin_amdgcn_sched_barrier(0);
      mma(na, nb0, nb1);
    }

    // epilogue: v = (exact level sum, rounded once) x 2^(row scale); sum of v^2 over the wave's rows in register order
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
      const double sc = p.wscale[row];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        int32_t lv[S];
#pragma unroll
        for (int l = 0; l < S; ++l) lv[l] = acc[c][l][i];
        const double v = i8_combine<S>(lv) * sc;
        ss[c] = fma(v, v, ss[c]);
        __builtin_amdgcn_sched_barrier(0);   // one output at a time: hoisting all 224 accumulator reads spills
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double o = __shfl_xor(ss[c], 32);
    if (lane < 32) red[wave][c * 32 + lane] = ss[c] + o;   // rows 4 h + ...: lane half 0's sum + half 1's
  }
  __syncthreads();
  if (tid < I8_CANDS) {
    const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    p.part[(int64_t)r * p.Mp + p.m0 + (int64_t)ct * I8_CANDS + tid] = v;
  }
}

// ---- dispatch ---------------------------------------------------------------------------------------------------------
// SlabI8 (posterior_plan.h): the slab walk of launch_posterior_slab, but the slab is S bytes per element and its width comes from
// i8_slab_width: small enough that the 32 row chunks re-read it from the 256 MB Infinity Cache rather than from HBM, and such that
// the generation's grid ends with the device's compute units full (GPBO_KSTAR_GB still caps it).  The byte bound I8_SLAB_BYTES is
// a constant of the rule: the debug build's slab-size switch (GPBO_I8_SLAB_MB, which produced the table quoted there) went with
// the plain byte rule, so another bound is probed by rebuilding.
int launch_posterior_slab_i8(gpbo_ctx* ctx, Model& m, int64_t Mp, const PostPlan& plan) {
  if (m.NP > I8_NP_MAX || m.NP % 64) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "posterior: the int8 GEMM serves NP <= 16384");
  int rc;
  if (!m.wd_valid && (rc = pack_wd(ctx, m))) return rc;
  const int64_t per_cand = m.NP * I8_S;          // bytes of one candidate's digit planes
  if (!ctx->compute_units) GPBO_HIP(ctx, hipDeviceGetAttribute(&ctx->compute_units, hipDeviceAttributeMultiprocessorCount, ctx->device));
  // no cap: the kernel's buffer offsets start at its own candidate tile
  const int64_t ms = i8_slab_width(m.NP, per_cand, kstar_slab_width(ctx, Mp, per_cand, INT64_MAX), ctx->compute_units);
  if ((rc = ensure(ctx, &ctx->kst, &ctx->cap_kst, (ms * per_cand + 7) / 8))) return rc;
  for (int64_t m0 = 0; m0 < Mp; m0 += ms) {
    const int64_t ldk = (Mp - m0 < ms) ? (Mp - m0) : ms;
    if ((rc = launch_kstar_digits(ctx, m, ctx->kst, ldk, Mp, m0, plan.mu_chunks))) return rc;
    I8Args a;
    a.Wd = m.Wd; a.wscale = m.wscale; a.Kd = reinterpret_cast<const uint4*>(ctx->kst); a.part = ctx->part;
    a.NP = (int)m.NP; a.Mp = Mp; a.nchunks = plan.part_chunks; a.n_ctiles = (int)(ldk / I8_CANDS); a.m0 = m0;
    const int64_t nblocks = (int64_t)a.n_ctiles * a.nchunks;
    posterior_i8_kernel<I8_S><<<dim3((unsigned)nblocks), dim3(256), 0, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
  }
  return GPBO_OK;
}

}  // namespace gpbo
