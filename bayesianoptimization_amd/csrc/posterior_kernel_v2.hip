// posterior_kernel_v2 — the posterior MFMA kernel tiled for FOUR waves per SIMD (v1, 2 waves/SIMD, is in the git
// history), with the k* operand either generated in-kernel (GEN = 1: the Fused256 / Fused512 paths of posterior_plan.h) or
// read from a slab (GEN = 2: SlabF64) — and kstar_gen_kernel, which writes the slab of every slab path.
//
// Why: the in-tree probe (gpbo_mfma_f64_probe) shows that on gfx950 a SIMD only reaches the
// 64-cycle issue cadence of v_mfma_f64_16x16x4_f64 when >= 4 waves feed it (1 wave: 140 cycles per
// MFMA, 2 waves: 102, 4 waves: 63), and rocprofv3 puts v1 (256 VGPRs -> 2 waves/SIMD) at 56 % matrix-pipe
// busy.  v2 halves the per-wave accumulator tile so that a wave fits 128 VGPRs:
//
//   workgroup = 8 waves, 256 rows of W x 64 candidates, two workgroups resident per CU (4 waves/SIMD);
//   wave w    = 32 rows x 64 candidates = 2 x 4 MFMA tiles = 64 accumulator VGPRs;
//   k* stage  = 16 train points x 64 candidates, 2 elements per thread (lane = candidate, wave = k pair),
//               candidate coordinates read from an LDS image (no registers to spare for them);
//   W slab    = streamed HBM/L2 -> registers in fragment order, prefetched one k-pair (8 columns) ahead.
//
// Same math, same reduction order per row chunk as v1 up to the candidate-tile width; results are
// deterministic.  Replaces the same reference lines as posterior_kernel.hip (_gpr.py:443-494).
#include <type_traits>

#include "gpbo_internal.h"
#include "fit_bodies.h"
#include "i8_digits.h"
#include "posterior_tile.h"

namespace gpbo {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int V2_CANDS = 64;
// Stage tile in LDS: [k-quad q][candidate group jt (16)][k in quad (4)][candidate in group (16)] doubles, i.e. blocks of
// 64 doubles = 512 B holding exactly what ONE B-fragment read of v_mfma_f64_16x16x4_f64 takes (lane l -> element l of
// block (q, jt)).  Every read of a stage — and of both stage buffers — is then the lane's own constant address plus a
// multiple of 512 B, which ds_read2st64_b64 carries as an immediate: no address arithmetic per read, and a wave reads
// 512 contiguous bytes (no bank conflicts).  (Round 1: [k][80] rows: 12 VALU instructions per stage for addresses.)
constexpr int V2_STRIDE = 64;  // doubles per k-row equivalent: a stage of BK points takes BK * 64 doubles

struct PostArgs2 {
  const double* Wp;
  const double* Xs;
  const double* alpha;
  const double* Xcs;
  double* part;
  double* mu_part;
  PostGrid g;
  const double* Kst;   // GEN == 2: materialised k* slab [NP][ldk], candidate-contiguous
  int64_t ldk;
  int64_t m0;          // first candidate of the slab (outputs are indexed m0 + local)
  int fuse_ends = 0;   // GEN == 1, one row chunk: raw candidates in, mu / sd out (PostEnds, gpbo_internal.h)
  PostEnds ends = {};
};

// GEN = 1: k* generated in the kernel (fused).  GEN = 2: k* read from a slab materialised by
// kstar_gen_kernel (the fp64 VALU work of the generation shares the FP64 datapath with the MFMAs — measured:
// 31 % of the fused kernel's time at C3 — so paying it once per candidate instead of once per row chunk wins).
// BK = train points per LDS stage (one s_barrier per stage): 16, or 32 for the slab kernel (half the barriers; the
// triangular cut-off of a 16-row tile then rounds up to 32 columns — zeros of the packed W, a few per cent more MFMAs
// in the diagonal chunk only).
// WAVES = 8: 256-row chunks, two workgroups per CU.  WAVES = 16 (round 4, GEN = 1 only, Fused512): 512-row chunks, ONE 1024-thread
// workgroup per CU — for NP <= 1024 a candidate tile's k* is then generated once (NP <= 512) or 1.5 times (NP <= 1024)
// instead of once per 256-row chunk (1.5 / 2.5 times) and never crosses HBM: the slab route generates it once too, but pays a
// 268 MB round trip at N = 512, M = 65 536 and a second launch (C2: 0.09 + 0.29 ms).
template <int DP, int KERNEL, int GEN, int BK = POST_BK, int WAVES = 8>
__global__ __launch_bounds__(WAVES * 64, 4) void posterior_kernel_v2(PostArgs2 p) {
  static_assert(GEN == 1 || GEN == 2, "k* generated in the kernel or read from a slab");
  static_assert(BK == 16 || BK == 32, "stages of 16 or 32 train points");
  static_assert(WAVES == 8 || (WAVES == 16 && GEN == 1 && BK == 32), "the 16-wave form is the fused kernel with 32-point stages");
  constexpr int NT = WAVES * 64;                   // threads
  constexpr int ROWS = WAVES * 32;                 // rows of W per workgroup (wave = two 16-row tiles)
  constexpr int E = BK / WAVES;                    // stage elements per thread (lane = candidate, wave = E train points)
  static_assert(GEN == 2 || E == 2 || E == 4, "the in-kernel generation computes train points in pairs: one or two pairs per thread and stage");
  constexpr int KP = BK / 8;                       // k-pairs (8 columns of W) per stage
  extern __shared__ __attribute__((aligned(16))) double smem2[];
  double* Ks = smem2;                              // [2][BK][V2_STRIDE]
  double* Xl = smem2 + 2 * BK * V2_STRIDE;         // [DP][64] candidate coordinates, dimension-major

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  int r, ct;
  p.g.map(blockIdx.x, r, ct);
  const bool last = (r == p.g.nchunks - 1);
  const int NP = p.g.NP;
  const int k_end = min(NP, (r + 1) * ROWS);
  const int n_stages = k_end / BK;

  // candidate tile -> LDS (thread t loads candidate t>>3, dims (t&7)*DP/8 ...)
  if constexpr (GEN != 2) {
    if (p.fuse_ends) {
      // the raw tile, scaled on the way in: prescale_elem's element (row < M and t < d: X / length_scale, else 0), into LDS instead of memory
      for (int e = tid; e < V2_CANDS * DP; e += NT) {
        const int cnd = e / DP, t = e - cnd * DP;
        const int64_t row = (int64_t)ct * V2_CANDS + cnd;
        double v = 0.0;
        if (row < p.ends.M && t < p.ends.d) v = p.ends.Xc[row * p.ends.d + t] / p.ends.ls[t];
        Xl[t * V2_CANDS + cnd] = v;
      }
    } else {
      const double* src = p.Xcs + (int64_t)ct * V2_CANDS * DP;
      for (int e = tid; e < V2_CANDS * DP; e += NT) {
        const int cnd = e / DP, t = e - cnd * DP;
        Xl[t * V2_CANDS + cnd] = src[e];
      }
    }
  }

  // MFMA role.  A chunk holds 16 tiles of 16 rows; wave w owns tiles w and 15 - w (not two adjacent ones):
  // in the chunk's diagonal block a tile t only needs the stages up to its own rows, so the pairing gives
  // every wave the same (t+1) + (16-t) = 17 tile-stages of work instead of 3 ... 31.
  const int tileA = r * (ROWS / 16) + wave;                     // global 16-row tile index (the earlier one)
  const int tileB = r * (ROWS / 16) + (2 * WAVES - 1) - wave;   // the later one
  const int rowA0 = tileA * 16, rowB0 = tileB * 16;
  const bool activeA = rowA0 < NP, activeB = rowB0 < NP;    // false only in a ragged last chunk
  const int64_t pairs = NP / 8;
  // packed W: [slab of 32 rows][k-pair][tile of 16 rows][lane] double2 ; inactive tiles stream tile 0 (dropped later)
  const int tA = activeA ? tileA : 0, tB = activeB ? tileB : 0;
  // Both operand streams are read through buffer descriptors: wave-uniform base in SGPRs, the lane as a constant 32-bit
  // offset, the walk along k as the instruction's scalar offset — no per-lane 64-bit address arithmetic in the MFMA loop
  // (12 v_lshl_add_u64 per stage with flat global loads; fp64 MFMAs and other VALU work do not overlap on this part).
  const double2* wpA = reinterpret_cast<const double2*>(p.Wp) + ((int64_t)(tA >> 1) * pairs * 2 + (tA & 1)) * 64;
  const double2* wpB = reinterpret_cast<const double2*>(p.Wp) + ((int64_t)(tB >> 1) * pairs * 2 + (tB & 1)) * 64;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<double2*>(wpA), 0, 0x7fffffff, BUF_FLAGS);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<double2*>(wpB), 0, 0x7fffffff, BUF_FLAGS);
  const unsigned voff16 = (unsigned)lane * 16u, voff8 = (unsigned)lane * 8u;

  d4 acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = d4{0.0, 0.0, 0.0, 0.0};
  double mu_acc = 0.0;

  // generation role: candidate = lane, train points E*wave .. E*wave + E - 1 of the stage
  auto gen_compute = [&](int stage, double (&kv)[E], double mu_weight) {
    const int j0 = stage * BK + wave * E;
    if constexpr (GEN == 2) {
      const double* src = p.Kst + (int64_t)j0 * p.ldk + (int64_t)ct * V2_CANDS;       // wave-uniform
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(src), 0, 0x7fffffff, BUF_FLAGS);
      const unsigned row = (unsigned)p.ldk * 8u;                                       // ldk * 8 * (E - 1) < 2^31 (slab budget)
#pragma unroll
      for (int e = 0; e < E; ++e)
        kv[e] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff8, (unsigned)e * row, 0));
      return;
    }
#pragma unroll
    for (int e2 = 0; e2 < E; e2 += 2) {
      const double* xr = p.Xs + (int64_t)(j0 + e2) * DP;  // wave-uniform -> scalar loads
      double d2a = 0.0, d2b = 0.0;
      if constexpr (DP <= 8) {
#pragma unroll
        for (int t = 0; t < DP; ++t) {
          const double x = Xl[t * V2_CANDS + lane];
          const double da = x - xr[t], db = x - xr[DP + t];
          d2a = fma(da, da, d2a);
          d2b = fma(db, db, d2b);
        }
      } else {
#pragma unroll 1
        for (int tb = 0; tb < DP; tb += 8) {
#pragma unroll
          for (int tt = 0; tt < 8; ++tt) {
            const double x = Xl[(tb + tt) * V2_CANDS + lane];
            const double da = x - xr[tb + tt], db = x - xr[DP + tb + tt];
            d2a = fma(da, da, d2a);
            d2b = fma(db, db, d2b);
          }
        }
      }
      kv[e2] = gpbo_kernel_value<KERNEL>(d2a);
      // (16 waves = 128 VGPRs: with DP = 4 the two inlined evaluations, interleaved, spilled 15-29 registers; one after the other fits)
      if constexpr (WAVES == 16 && (DP <= 4 || E > 2)) __builtin_amdgcn_sched_barrier(0);
      kv[e2 + 1] = gpbo_kernel_value<KERNEL>(d2b);
      if constexpr (WAVES == 16 && (DP <= 4 || E > 2)) __builtin_amdgcn_sched_barrier(0);
      // mu_weight = 0 for the clamped (repeated) look-ahead of the last stage: it must not be counted twice
      mu_acc = fma(kv[e2] * mu_weight, p.alpha[j0 + e2], mu_acc);
      mu_acc = fma(kv[e2 + 1] * mu_weight, p.alpha[j0 + e2 + 1], mu_acc);
    }
  };
  auto gen_store = [&](const double (&kv)[E], int buf) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int k = wave * E + e;     // train point of the stage this thread generated / fetched for candidate `lane`
      Ks[((buf * (BK / 4) + (k >> 2)) * 4 + (lane >> 4)) * 64 + (k & 3) * 16 + (lane & 15)] = kv[e];
    }
  };

  // A fragments for one k-pair (8 columns): [tile] double2 = 8 VGPRs
  auto loadA = [&](int kpair, double2(&a)[2]) {
    a[0] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rsA, voff16, (unsigned)kpair * 2048u, 0));
    a[1] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rsB, voff16, (unsigned)kpair * 2048u, 0));
  };
  // MODE 2: both tiles, 1: only the later tile (B), compile-time so that the hot loop stays one basic block
  auto mma_pair = [&](int buf, int pp, const double2(&a)[2], auto mode) {
    constexpr int MODE = decltype(mode)::value;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int q = pp * 2 + e;
      const double a0 = e ? a[0].y : a[0].x;
      const double a1 = e ? a[1].y : a[1].x;
      const double* kb = Ks + (buf * (BK / 4) + q) * 256 + lane;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const double b = kb[jt * 64];
        if constexpr (MODE == 2) acc[0][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][jt], 0, 0, 0);
        acc[1][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][jt], 0, 0, 0);
      }
    }
  };
  using both_t = std::integral_constant<int, 2>;
  using later_t = std::integral_constant<int, 1>;

  __syncthreads();   // Xl visible
  {
    double kv0[E];
    gen_compute(0, kv0, 1.0);
    gen_store(kv0, 0);
  }
  double2 aA[2], aB[2];
  loadA(0, aA);
  __syncthreads();

  // One stage = BK train points.  MODE 2: both tiles multiply, 1: only the later tile, 0: none (the wave only
  // feeds the stage tile).  The body is branch-free (the look-ahead indices are clamped instead of tested) so that
  // loads, MFMAs and the LDS store of a stage stay in one basic block.
  const int last_stage = n_stages - 1;
  const int last_pair = (int)pairs - 1;
  auto stage = [&](int st, auto mode) {
    constexpr int MODE = decltype(mode)::value;
    const int buf = st & 1;
    double kv[E];
    if constexpr (MODE > 0) loadA(min(KP * st + 1, last_pair), aB);
    gen_compute(min(st + 1, last_stage), kv, st < last_stage ? 1.0 : 0.0);
    // slab mode: these are plain global loads — keep them at the top of the stage (a full stage of MFMAs hides
    // their latency); without the fence hipcc sinks them next to their first use
    if constexpr (GEN == 2) __builtin_amdgcn_sched_barrier(0);
    // k-pairs alternate between the two fragment registers; each is refilled (two pairs ahead) right after its use —
    // the last one of the stage at the top of the next stage
    if constexpr (MODE > 0) {
#pragma unroll
      for (int pp = 0; pp < KP; ++pp) {
        if (pp & 1) mma_pair(buf, pp, aB, mode);
        else mma_pair(buf, pp, aA, mode);
        if (pp + 1 < KP || (pp & 1) == 0) {
          if (pp & 1) loadA(min(KP * st + pp + 2, last_pair), aB);
          else loadA(min(KP * st + pp + 2, last_pair), aA);
        }
      }
    }
    gen_store(kv, buf ^ 1);   // after the last LDS read of this stage (for st == last_stage nobody reads it)
    __syncthreads();
  };
  // stages 0 .. sA: both tiles; sA+1 .. sB: the later tile only; beyond: none (W is lower triangular)
  const int sA = min(last_stage, (rowA0 + 15) / BK);
  const int sB = min(last_stage, (rowB0 + 15) / BK);
  int s = 0;
  for (; s <= sA; ++s) stage(s, both_t{});
  for (; s <= sB; ++s) stage(s, later_t{});
  for (; s <= last_stage; ++s) stage(s, std::integral_constant<int, 0>{});

  // epilogue: per-candidate sum of squares over this chunk's rows, fixed order
  static_assert(2 * WAVES * V2_CANDS <= 2 * BK * V2_STRIDE, "the epilogue's exchange area aliases the stage tiles");
  double* red = Ks;                           // [WAVES][64]
  double* mured = Ks + WAVES * V2_CANDS;      // [WAVES][64]
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    double v = 0.0;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) v = fma(acc[0][jt][rr], acc[0][jt][rr], v);
    if (!activeA) v = 0.0;
    double vb = 0.0;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) vb = fma(acc[1][jt][rr], acc[1][jt][rr], vb);
    if (activeB) v += vb;
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lane < 16) red[wave * V2_CANDS + jt * 16 + lane] = v;
  }
  mured[wave * V2_CANDS + lane] = mu_acc;
  __syncthreads();
  if (tid < V2_CANDS) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) v += red[w * V2_CANDS + tid];
    const int64_t m = p.m0 + (int64_t)ct * V2_CANDS + tid;
    if (GEN != 2 && p.fuse_ends) {
      // this workgroup holds every row of its candidates: mu and sd from here (what posterior_finalize_kernel makes of ONE partial
      // each: 0.0 + v and 0.0 + u are v and u)
      double u = 0.0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) u += mured[w * V2_CANDS + tid];
      if (m < p.ends.M)
        posterior_finalize_elem(0.0 + v, 0.0 + u, p.ends.y_mean, p.ends.y_std, p.ends.amplitude, p.ends.white, p.ends.mu + m, p.ends.sd + m, p.ends.negvar);
      return;
    }
    p.part[(int64_t)r * p.g.Mp + m] = v;
    if (GEN != 2 && last) {
      double u = 0.0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) u += mured[w * V2_CANDS + tid];
      p.mu_part[m] = u;
    }
  }
}

// k* slab generation: thread = candidate (coordinates in registers), loop over a chunk of 256 train points; also the partial
// means sum_k k*[k] alpha[k] per chunk.  The train points of the chunk are staged through LDS 64 at a time and read back as
// broadcasts (every lane the same address): as scalar loads straight from memory each pair of points cost the wave four
// s_load_dwordx16 + s_waitcnt round trips per iteration, which left the fp64 VALU — the unit this kernel is bound by — idle about
// 40 % of the time (14.2 ms per C3 pass).
// SLAB = the slab path (posterior_plan.h) names what the slab holds; the k* values and the partial means are the same for all:
//   SlabF64  the values, Kst[k][m] (candidate-contiguous: coalesced stores);
//   SlabF32  the values ROUNDED to fp32 (half the HBM traffic; the means are accumulated in fp64 before the rounding);
//   SlabI8   their I8_S int8 digit planes (i8_digits.h) in the operand order of v_mfma_i32_16x16x64_i8 (i8_frag_index) — [candidate
//            block of 16][64 train points][plane][lane] 16 bytes, lane 16 g + c = candidate c, train points 16 g ... 16 g + 15 —
//            written as one 16-byte store per plane and 16 train points: a wave's store instruction is 1 KiB, four candidate
//            blocks of 256 contiguous bytes (two whole lines) each.
constexpr int GEN_CH = 64;
template <PostPath SLAB> struct slab_value { using type = double; };
template <> struct slab_value<PostPath::SlabF32> { using type = float; };
template <int DP, int KERNEL, PostPath SLAB>
__global__ __launch_bounds__(256) void kstar_gen_kernel(const double* __restrict__ Xs, const double* __restrict__ alpha,
                                                        const double* __restrict__ Xcs, void* __restrict__ slab,
                                                        int64_t ldk, int NP, double* __restrict__ mu_part,
                                                        int64_t Mp, int64_t m0) {
  static_assert(SLAB == PostPath::SlabF64 || SLAB == PostPath::SlabF32 || SLAB == PostPath::SlabI8, "a slab path");
  __shared__ __attribute__((aligned(16))) double xs[GEN_CH * DP];
  __shared__ double al[GEN_CH];
  const int64_t ml = (int64_t)blockIdx.x * 256 + threadIdx.x;   // slab-local candidate
  const bool live = ml < ldk;
  const int k0 = blockIdx.y * POST_ROWS, k1 = min(NP, k0 + POST_ROWS);
  double xc[DP];
  {
    const double* xcp = Xcs + (m0 + (live ? ml : 0)) * DP;
#pragma unroll
    for (int t = 0; t < DP; t += 2) {
      const double2 v = *reinterpret_cast<const double2*>(xcp + t);
      xc[t] = v.x;
      xc[t + 1] = v.y;
    }
  }
  double mu = 0.0;
  // k* of the staged train points kk, kk + 1, and their share of the mean (ka then kb, ascending k).  Two steps, so that each
  // form keeps the mean's fmas where its schedule had them: behind the value forms' stores, in front of the digit form's split.
  auto pair = [&](int kk, double& ka, double& kb) {
    const double* xr = xs + kk * DP;           // the same address in every lane: LDS broadcast
    double d2a = 0.0, d2b = 0.0;
#pragma unroll
    for (int t = 0; t < DP; ++t) {
      const double da = xc[t] - xr[t], db = xc[t] - xr[DP + t];
      d2a = fma(da, da, d2a);
      d2b = fma(db, db, d2b);
    }
    ka = gpbo_kernel_value<KERNEL>(d2a);
    kb = gpbo_kernel_value<KERNEL>(d2b);
  };
  auto mean = [&](int kk, double ka, double kb) {
    mu = fma(ka, al[kk], mu);
    mu = fma(kb, al[kk + 1], mu);
  };
  for (int kc = k0; kc < k1; kc += GEN_CH) {      // NP is a multiple of 64: every refill is full
    __syncthreads();
    {
      const double2* src = reinterpret_cast<const double2*>(Xs + (int64_t)kc * DP);
      double2* dst = reinterpret_cast<double2*>(xs);
      for (int e = threadIdx.x; e < GEN_CH * DP / 2; e += 256) dst[e] = src[e];
      if (threadIdx.x < GEN_CH) al[threadIdx.x] = alpha[kc + threadIdx.x];
    }
    __syncthreads();
    if (!live) continue;
    if constexpr (SLAB == PostPath::SlabI8) {
      // 16 train points at a time: the digit planes of 16 k* values are one 16-byte operand chunk per plane
      constexpr int S = I8_S;
      uint4* Kd = static_cast<uint4*>(slab);
      const int64_t cb = i8_kd_block(ml >> 4, NP);
#pragma unroll 1
      for (int kg = 0; kg < GEN_CH; kg += 16) {
        uint32_t w[S][4] = {};
#pragma unroll
        for (int kk = kg; kk < kg + 16; kk += 2) {
          double ka, kb;
          pair(kk, ka, kb);
          mean(kk, ka, kb);
          const int64_t qa = i8_quantize<S>(ka), qb = i8_quantize<S>(kb);
          const int j = kk - kg;
#pragma unroll
          for (int t = 0; t < S; ++t) {
            w[t][j >> 2] |= (uint32_t)((qa >> (8 * (S - 1 - t))) & 255) << (8 * (j & 3));
            w[t][j >> 2] |= (uint32_t)((qb >> (8 * (S - 1 - t))) & 255) << (8 * ((j + 1) & 3));
          }
        }
        const int k = kc + kg;   // multiple of 16
        uint4* dst = Kd + i8_frag_index<S>(cb, k, 0, (int)(ml & 15));
#pragma unroll
        for (int t = 0; t < S; ++t) {
          const uint32_t x = t ? 0x80808080u : 0u;   // planes below the leading one: byte - 128 (i8_digit_byte)
          dst[t * 64] = make_uint4(w[t][0] ^ x, w[t][1] ^ x, w[t][2] ^ x, w[t][3] ^ x);
        }
      }
    } else {
      using T = typename slab_value<SLAB>::type;
      T* Kst = static_cast<T*>(slab);
#pragma unroll 2
      for (int kk = 0; kk < GEN_CH; kk += 2) {
        double ka, kb;
        pair(kk, ka, kb);
        const int k = kc + kk;
        Kst[(int64_t)k * ldk + ml] = (T)ka;
        Kst[(int64_t)(k + 1) * ldk + ml] = (T)kb;
        mean(kk, ka, kb);
      }
    }
  }
  if (live) mu_part[(int64_t)blockIdx.y * Mp + m0 + ml] = mu;
}

template <PostPath SLAB>
static int launch_gen(gpbo_ctx* ctx, Model& m, void* slab, int64_t ldk, int64_t Mp, int64_t m0, int nchunks) {
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    kstar_gen_kernel<decltype(dp)::value, decltype(k)::value, SLAB><<<dim3((unsigned)((ldk + 255) / 256), (unsigned)nchunks), dim3(256), 0,
                                                                      ctx->stream>>>(m.Xs, m.alpha, ctx->Xcs, slab, ldk, (int)m.NP,
                                                                                     ctx->mu_part, Mp, m0);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

// The slab for candidates [m0, m0 + ldk) of the scaled set ctx->Xcs + their partial means in ctx->mu_part [nchunks][Mp]:
// k* [NP][ldk] — also used by the covariance path (posterior_cov.hip) —
int launch_kstar_slab(gpbo_ctx* ctx, Model& m, double* Kst, int64_t ldk, int64_t Mp, int64_t m0, int nchunks) {
  return launch_gen<PostPath::SlabF64>(ctx, m, Kst, ldk, Mp, m0, nchunks);
}
// ... the same rounded to fp32,
int launch_kstar_slab_f32(gpbo_ctx* ctx, Model& m, float* Kst, int64_t ldk, int64_t Mp, int64_t m0, int nchunks) {
  return launch_gen<PostPath::SlabF32>(ctx, m, Kst, ldk, Mp, m0, nchunks);
}
// ... its I8_S int8 digit planes (ldk a multiple of 32)
int launch_kstar_digits(gpbo_ctx* ctx, Model& m, void* Kd, int64_t ldk, int64_t Mp, int64_t m0, int nchunks) {
  return launch_gen<PostPath::SlabI8>(ctx, m, Kd, ldk, Mp, m0, nchunks);
}

// The kernel's arguments for ncands candidates in nchunks row chunks (no slab, no fused ends).
static PostArgs2 post_args(gpbo_ctx* ctx, const Model& m, int64_t Mp, int nchunks, int64_t ncands) {
  PostArgs2 a;
  a.Wp = m.Wp; a.Xs = m.Xs; a.alpha = m.alpha; a.Xcs = ctx->Xcs; a.part = ctx->part; a.mu_part = ctx->mu_part;
  a.g = {(int)m.NP, Mp, nchunks, (int)(ncands / V2_CANDS)};
  a.Kst = nullptr; a.ldk = 0; a.m0 = 0;
  return a;
}

// SlabF64's GEMM for one slab of the walk (launch_posterior_slabs): posterior_kernel_v2<.., GEN = 2>.  32 train points per stage:
// 262.9 vs 264.0 ms per C3 launch (round-2 A/B).
int launch_slab_gemm_f64(gpbo_ctx* ctx, Model& m, const double* slab, int64_t ldk, int64_t m0, int64_t Mp, int part_chunks) {
  PostArgs2 a = post_args(ctx, m, Mp, part_chunks, ldk);
  a.Kst = slab; a.ldk = ldk; a.m0 = m0;
  const size_t lds = (size_t)(2 * 32 * V2_STRIDE) * sizeof(double);
  posterior_kernel_v2<4, 0, 2, 32><<<dim3((unsigned)a.g.blocks()), dim3(512), lds, ctx->stream>>>(a);
  GPBO_HIP(ctx, hipGetLastError());
  return GPBO_OK;
}

// Fused256 (8 waves, 256-row chunks) and Fused512 (16 waves, 512-row chunks; NP <= 1024: at most two), the ends fused when
// the plan says so (one row chunk).  Mp must be a multiple of 64.
int launch_posterior_fused(gpbo_ctx* ctx, Model& m, int64_t Mp, const PostPlan& plan, const PostEnds& ends) {
  if (plan.fuse_ends && plan.part_chunks != 1) GPBO_FAIL(ctx, GPBO_ERR_STATE, "posterior: fused ends need one row chunk");
  PostArgs2 a = post_args(ctx, m, Mp, plan.part_chunks, Mp);
  const int64_t nblocks = a.g.blocks();
  if (nblocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "posterior: grid too large; shard the candidates");
  if (plan.fuse_ends) { a.fuse_ends = 1; a.ends = ends; }
  const bool wide = plan.path == PostPath::Fused512;
  return with_dp_kernel(ctx, m.DP, m.kernel, [&](auto dp, auto k) {
    constexpr int DP = decltype(dp)::value, KERNEL = decltype(k)::value;
    if (wide) {
      const size_t lds = (size_t)(2 * 32 * V2_STRIDE + DP * V2_CANDS) * sizeof(double);
      posterior_kernel_v2<DP, KERNEL, 1, 32, 16><<<dim3((unsigned)nblocks), dim3(1024), lds, ctx->stream>>>(a);
    } else {
      const size_t lds = (size_t)(2 * POST_BK * V2_STRIDE + DP * V2_CANDS) * sizeof(double);
      posterior_kernel_v2<DP, KERNEL, 1><<<dim3((unsigned)nblocks), dim3(512), lds, ctx->stream>>>(a);
    }
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
}

}  // namespace gpbo

#ifdef GPBO_DEBUG   // the k* generation alone, both branches side by side (include/gpbo.h, "debug build"): tests/test_gpu_int8_exact.py
using namespace gpbo;

int gpbo_debug_i8_kstar_digits(gpbo_ctx* ctx, int64_t NP, int64_t m0, int64_t ldk, void* Kd_out, double* kst_out, double* mu_part_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  Model& m = ctx->models[0];
  if (!m.fitted || ctx->pending_info[0]) GPBO_FAIL(ctx, GPBO_ERR_STATE, "debug_i8_kstar_digits: model slot 0 has not been fitted");
  if (ctx->M < 1) GPBO_FAIL(ctx, GPBO_ERR_STATE, "debug_i8_kstar_digits: no candidates resident (call gpbo_set_candidates)");
  if (ctx->d_c != m.d) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_i8_kstar_digits: candidate dimension differs from the fitted model");
  const int64_t Mp = round_up(ctx->M, POST_CANDS);
  if (!Kd_out || !kst_out || !mu_part_out || m0 < 0 || ldk < 64 || m0 % 64 || ldk % 64 || m0 + ldk > Mp)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_i8_kstar_digits: bad arguments (m0, ldk multiples of 64 inside the padded candidate set)");
  if (m.NP > I8_NP_MAX || m.NP % 64) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "debug_i8_kstar_digits: the int8 GEMM serves NP <= 16384");
  if (NP != m.NP)   // the caller sized its buffers from NP: refuse before anything is written
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "debug_i8_kstar_digits: NP is not the padded size of the model in slot 0");
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  const int nchunks = (int)((m.NP + POST_ROWS - 1) / POST_ROWS);
  int rc;
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * m.DP))) return rc;
  if ((rc = ensure(ctx, &ctx->mu_part, &ctx->cap_mu_part, (int64_t)nchunks * Mp))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, ctx->M, m.d, m.DP, m.ls, ctx->Xcs, Mp))) return rc;
  const size_t kd_bytes = (size_t)ldk * m.NP * I8_S, kst_bytes = (size_t)ldk * m.NP * sizeof(double);
  void* dKd = nullptr;     // slabs of their own: the context's slab workspace keeps its size
  double* dKst = nullptr;
  auto done = [&](int code) {
    if (dKd) (void)hipFree(dKd);
    if (dKst) (void)hipFree(dKst);
    return code;
  };
  if (hipMalloc(&dKd, kd_bytes) != hipSuccess || hipMalloc((void**)&dKst, kst_bytes) != hipSuccess) return done(GPBO_ERR_HIP);
  for (int which = 0; which < 2; ++which) {   // 0: the digit branch, 1: the fp64 branch; the partial means of each
    rc = which ? launch_kstar_slab(ctx, m, dKst, ldk, Mp, m0, nchunks) : launch_kstar_digits(ctx, m, dKd, ldk, Mp, m0, nchunks);
    if (rc) return done(rc);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return done(GPBO_ERR_HIP);
    for (int q = 0; q < nchunks; ++q)
      if (hipMemcpy(mu_part_out + ((int64_t)which * nchunks + q) * ldk, ctx->mu_part + (int64_t)q * Mp + m0, (size_t)ldk * sizeof(double),
                    hipMemcpyDeviceToHost) != hipSuccess)
        return done(GPBO_ERR_HIP);
  }
  if (hipMemcpy(Kd_out, dKd, kd_bytes, hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  if (hipMemcpy(kst_out, dKst, kst_bytes, hipMemcpyDeviceToHost) != hipSuccess) return done(GPBO_ERR_HIP);
  return done(GPBO_OK);
}
#endif  // GPBO_DEBUG
