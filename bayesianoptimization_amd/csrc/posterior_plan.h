// Which device path a posterior pass takes (posterior_kernel.hip's launch_posterior), as a pure function of plain values.
// Host-only and free of HIP: tests/test_posterior_plan_host.py compiles it with the system C++ compiler and pins the rule on
// both sides of every edge.  The debug switches (GPBO_POST_KERNEL, GPBO_POST_SMALL, GPBO_POST_FUSE_ENDS) are read by the caller
// and come in already parsed.
#pragma once

#include <cstdint>

namespace gpbo {

constexpr int POST_ROWS = 256;       // W rows owned by one posterior workgroup (8 waves x 32 rows)
constexpr int POST_ROWS_WIDE = 512;  // ... by the 16-wave fused kernel and by the fp32 kernel on 32x32 MFMAs
constexpr int POST_CANDS = 128;      // candidate padding granule (Mp = round_up(M, 128); kernels tile 64 candidates)
constexpr int I8_ROWS = 128;         // rows of W per workgroup of the int8 GEMM (4 waves x 32)
constexpr int64_t I8_NP_MIN = 2048;  // fp64 models take the int8 GEMM from this NP on ...
constexpr int I8_NP_MAX = 16384;     // ... up to this one: i8_digits.h's int32 level sums bound it
constexpr int I8_S = 7;              // int8 digit planes per operand (i8_digits.h): bytes per k* value of SlabI8's slab

enum class PostPath {
  Small,     // batched GEMV                                       posterior_small.hip
  Fused256,  // k* generated inside the MFMA kernel, 8 waves       posterior_kernel_v2.hip (GEN = 1)
  Fused512,  // ... 16 waves, 512-row chunks                       posterior_kernel_v2.hip (GEN = 1, WAVES = 16)
  // The slab paths: one walk (posterior_kernel.hip, launch_posterior_slabs) over slabs of slab_spec's size, per slab one launch
  // of kstar_gen_kernel<.., the path> (posterior_kernel_v2.hip) and one of the path's GEMM:
  SlabF64,   // k* slab + fp64 MFMA GEMM                           posterior_kernel_v2.hip (GEN = 2)
  SlabI8,    // k* slab as int8 digit planes + int8 MFMA GEMM      posterior_i8.hip
  SlabF32,   // fp32 k* slab + fp32 MFMA GEMM                      posterior_kernel_f32.hip
};

struct PostPlan {
  PostPath path;
  bool fuse_ends;   // the fused kernel takes the raw candidates and writes mu / sd itself: no prescale, no finalize launch
  int part_chunks;  // rows of sum-of-squares partials (ctx->part) the finalize kernel sums
  int mu_chunks;    // rows of mean partials (ctx->mu_part)
};

// The fp32 GEMM runs on v_mfma_f32_32x32x2_f32 in 512-row chunks from NP = 512 on, on v_mfma_f32_16x16x4_f32 in 256-row chunks
// below.  Same rate, same operand bytes per flop; the 32x32 form is half the MFMA instructions (64 cycles each instead of 32),
// which leaves the issue slots the LDS reads, the slab / W loads and the barrier need: the 16x16 kernel ran its matrix pipe 81 %
// busy.  The two forms want W packed differently (launch_pack_w32).
inline bool f32_use_mfma32(int64_t NP) { return NP >= POST_ROWS_WIDE; }

// fp64 models on the slab route take the int8 GEMM by NP alone, never by M, so that a candidate's mu / sd do not depend on the
// batch it comes in; the int32 level sums bound NP from above.
inline bool posterior_i8_serves(int64_t NP) { return NP >= I8_NP_MIN && NP <= I8_NP_MAX; }

// What the slab walk needs to know about a slab path's slab.  The workspace budget (kstar_slab_width) divided by bytes_per_cand
// gives the slab's width in candidates, at most offset_cap; a budget that holds fewer than 128 candidates fails the pass unless
// narrow_ok, which takes 128.
//   SlabF64, SlabF32: both value GEMMs address the rows of a stage as 32-bit buffer offsets from the stage's first row (ldk x 8
//   resp. 4 bytes apart: posterior_kernel_v2<.., GEN = 2>, posterior_kernel_f32x), so three rows of ldk values must stay below 2^31
//   bytes: 80e6 doubles, 160e6 floats.  A slab only has to be wide enough to fill the chip anyway (4e9 B = 121 984 candidates at
//   N = 4096 = 1906 candidate tiles x 16 row chunks per launch); measured at C3: one 34 GB slab 263.7 ms, eight 4 GB slabs 264.4 ms
//   (round 1 A/B) — the big workspace bought nothing.
//   SlabI8: no cap — the int8 GEMM's buffer offsets start at its own candidate tile; its width comes from i8_slab_width below.
struct SlabSpec {
  int64_t bytes_per_cand;   // of one candidate's NP k* values in the slab
  int64_t offset_cap;       // candidates
  bool narrow_ok;
};
inline SlabSpec slab_spec(PostPath path, int64_t NP) {
  switch (path) {
    case PostPath::SlabF64: return {8 * NP, (int64_t)80 * 1000 * 1000, false};
    case PostPath::SlabF32: return {4 * NP, (int64_t)160 * 1000 * 1000, false};
    case PostPath::SlabI8: return {I8_S * NP, INT64_MAX, true};
    default: return {0, 0, false};   // not a slab path
  }
}
// The slab buffer is counted in doubles: ms candidates take (ms * bytes_per_cand + 7) / 8 of them.  (8 NP bytes: ms * NP exactly;
// 4 NP bytes: x = ms * NP floats, (4 x + 7) / 8 = (x + 1) / 2 only because the division floors: x even gives x / 2, x odd (x + 1) / 2.)
inline int64_t slab_doubles(int64_t ms, int64_t bytes_per_cand) { return (ms * bytes_per_cand + 7) / 8; }

// SlabI8's slab width in candidates (one launch of kstar_gen_kernel<.., SlabI8> + one of the int8 GEMM per slab), from NP, the bytes of
// one candidate's digit planes (NP x S), the width the workspace budget grants (kstar_slab_width: a multiple of 128, <= Mp) and the
// device's compute units.
// Two things bound it.  The GEMM's 32 row chunks re-read the slab, so it has to stay in the 256 MB Infinity Cache (C3 pass per slab
// size, measured with the plain byte rule: 128 MB 204.4 ms, 256 MB 196.6, 512 MB 211.1, 1 GB 211.0, 4 GB 216.0).  And the generation's
// grid should end with the chip full: it launches ceil(width / 256) x ceil(NP / 256) equal workgroups at 1.3 - 1.5 waves per SIMD and
// lasts as long as the CUs that get one more than the others.  Below the byte bound, down to half of it, the rule takes the width (a
// multiple of 256) whose generation grid fills the largest share of its last round over the compute units, the widest one among
// equals.  The GEMM's grid (ceil(NP / 128) x width / 64 workgroups, one per CU) is 8 times the generation's when NP is a multiple of
// 256 and then ends full with it; its workgroups are of unequal cost (triangular, heaviest first), so for it "full" is an
// approximation, and at other NP (2112: 17 x 224 = 14.9 per CU) the rule does not look at it at all.
// C3 (NP = 4096, 16 chunks): 8928 candidates fit; 8832 (the plain multiple of 128) is 35 x 16 = 560 workgroups = 0.73 of three rounds,
// 8192 is 512 = exactly two.  Measured on one MI355X, plain rule -> this one, profiles/i8_lds_ab.json:
//   C3 kernel totals per pass, three alternating traced runs of 25 passes per arm (medians; ranges 0.15 / 0.15 and 0.86 / 0.53):
//     generation 23.15 -> 18.54 ms, GEMM 174.45 -> 171.76 ms (every run of the new arm below every run of the old one);
//     bench.py C3 on another box, three runs per arm: 193.5 -> 186.2 ms per step.
//   Posterior pass (M = 2^20, d = 16, medians of three), width and ms: NP = 1536: 23 808 -> 21 760, 35.9 -> 34.3;
//     2048: 17 792 -> 16 384, 57.2 -> 55.4;  2112 (9 chunks: 17 % more launches): 17 280 -> 14 336, 61.1 -> 59.8;
//     3072: 11 904 -> 10 752, 116.8 -> 113.2;  4096: 8832 -> 8192, 197.1 -> 189.4.
// Generating four slabs per launch instead (C3: 35 328 candidates, the GEMM walking sub-slabs of 8832) took the generation to 15.3 ms
// but cost the GEMM 4.9 ms: every sub-slab's first row chunk then reads its digits from HBM.
constexpr int64_t I8_SLAB_BYTES = 256 * 1000 * 1000;
inline int64_t i8_slab_width(int64_t NP, int64_t bytes_per_cand, int64_t granted, int64_t compute_units) {
  const int64_t chunks = (NP + POST_ROWS - 1) / POST_ROWS;
  const int64_t kmax = I8_SLAB_BYTES / bytes_per_cand / 256;
  int64_t width = I8_SLAB_BYTES / bytes_per_cand / 128 * 128;   // less than 256 candidates fit: the plain multiple of 128
  int64_t best_wgs = 0, best_cap = 1;
  for (int64_t k = kmax; k >= 1 && 2 * k > kmax; --k) {
    const int64_t wgs = k * chunks, cap = (wgs + compute_units - 1) / compute_units * compute_units;
    if (wgs * best_cap > best_wgs * cap) { best_wgs = wgs; best_cap = cap; width = 256 * k; }
  }
  if (granted < width) width = granted;
  return width < 128 ? 128 : width;   // below 128 candidates the walk still takes 128
}

// The rule: plan_posterior, first match wins (nchunks = 256-row chunks, Mp = M padded to 128, the GEMV limit small_batch_limit).
// Why.  The slab route as soon as k* would be generated more than once: the fp64 VALU work of the generation runs instead of
// MFMAs, not beside them, and the slab GEMM's loop carries no other VALU work.  For 384 <= NP <= 512 and a batch that fills the
// chip, Fused512 (round 4): ONE 16-wave workgroup covers all rows, so k* is generated once and never crosses HBM (the slab
// route: a 268 MB round trip and a second launch at C2).  Measured at M = 65 536 (scripts/r04_post_small_np_ab.py,
// profiles/r04_post_small_np_ab.json; round 2: scripts/archive/r02_small_n_posterior_ab.py), ms for Fused256 / SlabF64 / Fused512:
//   NP = 512, d = 8 : 0.406 / 0.374 / 0.352 (0.58 / 0.62 / 0.66 of the fp64 matrix peak)            -> Fused512
//   NP = 448, d = 8 : 0.357 / 0.332 / 0.327                                                         -> Fused512
//   NP = 1024, d = 16: 1.48 / 1.19 / 1.31 (two 512-row chunks: k* generated 1.5 times)               -> SlabF64
//   NP = 768, d = 16, M = 2^18: SlabF64 2.87, Fused512 4.72 (a ragged second chunk of 16 waves, half of them idle)
//   NP = 512, M = 8192: 0.073 / 0.115 / 0.087 (a grid of 128 workgroups does not fill the chip)    -> Fused256
//   NP = 256: Fused256 0.12 vs SlabF64 0.14 (one chunk: nothing is generated twice).
// Fused512 gains only 6 % where the slab traffic and a launch go away: its floor is the GEMM at the matrix pipe's 0.95 (0.25 ms)
// + one generation of k* on the same datapath (~0.09 ms); one 1024-thread workgroup per CU also means every s_barrier stalls the
// whole CU (the 16-wave slab kernel measured 3 % slower at C3 for the same reason).
// Two row chunks and a batch around bayes_opt's DEFAULT n_random = 10 000 (round 6, scripts/r06_post_10k_ab.py,
// profiles/r06_post_10k_ab.json; ms at M = 10 000 / 20 000 for N = 300, 384, 450, 512; SlabF64 was the rule's choice then):
//   SlabF64 0.125-0.147 / 0.16-0.19;  Fused256 0.092-0.113 / 0.12-0.17;  Fused512 0.080-0.100 / 0.14-0.18
// 144 ... 256 candidate tiles are one 16-wave workgroup per CU in ONE round; from there to 32 768 candidates the 8-wave kernel's
// two workgroups per CU fill the chip better than either.
// The int8 GEMM, ms per posterior pass, M = 2^20, d = 16, Matern-2.5 (debug build, GPBO_POST_KERNEL=3 | 8, one MI355X):
//   NP = 1536: SlabF64 40.0, SlabI8 35.9;  2048: 68.0 / 56.6;  3072: 145.7 / 116.5;  4096: 255.8 / 196.5.
// It wins from 1536 on; the rule starts at 2048, the smallest NP the suite checks it at (the ill-conditioned N = 2000 case of
// test_gpu_conditioning.py); NP <= 1024 keeps the fp64 kernels that the three-kernel parity test pins.
// A fused kernel whose workgroups hold ALL rows of their candidates (one row chunk) takes the raw candidates in and writes mu / sd
// itself (round 6: three launches -> one).
//
// Debug overrides (parsed by the caller): force_kernel = GPBO_POST_KERNEL's digit — 2 Fused256, 3 SlabF64 (always), 4 Fused512
// (NP <= 1024), 8 SlabI8 (512 < NP <= I8_NP_MAX); never for fp32 models, never past the Small row.  no_small: GPBO_POST_SMALL=0.
// no_fuse_ends: GPBO_POST_FUSE_ENDS=0 (the three launches).
inline PostPlan plan_posterior(int64_t NP, int64_t M, bool f32, int64_t gemv_limit, int force_kernel = 0, bool no_small = false,
                               bool no_fuse_ends = false) {
  const int nchunks = (int)((NP + POST_ROWS - 1) / POST_ROWS);
  const int64_t Mp = (M + POST_CANDS - 1) / POST_CANDS * POST_CANDS;
  if (M <= gemv_limit && !no_small) return {PostPath::Small, false, 0, 0};
  if (f32)
    return {PostPath::SlabF32, false, f32_use_mfma32(NP) ? (int)((NP + POST_ROWS_WIDE - 1) / POST_ROWS_WIDE) : nchunks, nchunks};
  PostPath path;
  if (nchunks <= 1) path = PostPath::Fused256;
  else if (nchunks == 2) {
    if (Mp < 8192) path = PostPath::Fused256;
    else if (Mp < 9216) path = PostPath::SlabF64;
    else if (Mp <= 16384) path = PostPath::Fused512;
    else if (Mp < 32768) path = PostPath::Fused256;
    else path = NP >= 384 ? PostPath::Fused512 : PostPath::SlabF64;
  } else path = posterior_i8_serves(NP) ? PostPath::SlabI8 : PostPath::SlabF64;
  switch (force_kernel) {
    case 2: path = PostPath::Fused256; break;
    case 3: path = PostPath::SlabF64; break;
    case 4: if (NP <= 1024) path = PostPath::Fused512; break;
    case 8: if (NP > 512 && NP <= I8_NP_MAX) path = PostPath::SlabI8; break;
  }
  PostPlan p{path, false, nchunks, nchunks};
  if (path == PostPath::Fused256 || path == PostPath::Fused512) {
    if (path == PostPath::Fused512) p.part_chunks = (int)((NP + POST_ROWS_WIDE - 1) / POST_ROWS_WIDE);
    p.mu_chunks = 1;
    p.fuse_ends = p.part_chunks == 1 && !no_fuse_ends;
  } else if (path == PostPath::SlabI8) {
    p.part_chunks = (int)((NP + I8_ROWS - 1) / I8_ROWS);
  }
  return p;
}

}  // namespace gpbo
