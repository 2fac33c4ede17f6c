// How gpmf_mes_argbest's pair pass (mfmes.hip) tiles its work, as pure functions of plain values.  Host-only and free of HIP:
// tests/test_mf_plan_host.py compiles it with the system C++ compiler and pins the edges.
//
// A workgroup of MF_WAVES = 8 waves owns MF_CANDS = 32 candidates and BOTH members of their pairs (z, z'), and walks every row
// chunk of W itself: MF_ROWS = 256 rows per chunk (16 tiles of 16 rows, two per wave), MF_BK = 16 train points per LDS stage.
// 32 pairs are four 16-column B fragments of v_mfma_f64_16x16x4_f64 — fragment 2 g + e is member e (0: z, 1: z') of candidate group
// g — so a wave's accumulators are 2 tiles x 4 fragments x 4 doubles = 64 registers, the posterior kernel's.  With the generation's
// registers (two kernel values and their stage-ahead staging) the instances take 177 - 197 VGPRs: two waves per SIMD, one workgroup
// per compute unit, no scratch.  Forced to 128 registers they spill 190 - 370 bytes per lane, so the bound is 2.  64 pairs per
// workgroup would need 128 accumulator registers per wave.
// There is no refusal rule: the walk serves every NP a slot can hold (NP a multiple of 64) and every M whose tiles fit a grid.
#pragma once

#include <cstdint>

namespace gpbo {

constexpr int MF_CANDS = 32;        // candidate pairs per workgroup
constexpr int MF_WAVES = 8;         // waves per workgroup
constexpr int MF_ROWS = 256;        // rows of W per chunk of the walk
constexpr int MF_BK = 16;           // train points per stage: one (candidate, point) per thread and stage
constexpr int MF_XS_PAD = 2;        // doubles behind a staged train point's DP coordinates (two points a wave: apart in the banks)
constexpr int MF_MAX_SAMPLES = 64;  // GPMF_MAX_SAMPLES

static_assert(MF_CANDS * MF_BK == MF_WAVES * 64, "a stage is one (candidate, train point) per thread");
static_assert(MF_ROWS == MF_WAVES * 32, "a chunk is two 16-row tiles per wave");

constexpr int mf_chunks(int64_t NP) { return (int)((NP + MF_ROWS - 1) / MF_ROWS); }
// stages a chunk walks: the triangular stop — chunk r ends at its last row
constexpr int mf_chunk_stages(int64_t NP, int r) {
  return (int)(((int64_t)(r + 1) * MF_ROWS < NP ? (int64_t)(r + 1) * MF_ROWS : NP) / MF_BK);
}
// the two tiles of wave w in chunk r (global 16-row tile indices): the pairing w, 15 - w gives every wave the same 17 tile-stages
// of the chunk's diagonal block
constexpr int mf_tile_a(int r, int w) { return r * (MF_ROWS / 16) + w; }
constexpr int mf_tile_b(int r, int w) { return r * (MF_ROWS / 16) + (2 * MF_WAVES - 1) - w; }
// the last stage tile t multiplies (W is lower triangular), clamped to the chunk's
constexpr int mf_tile_last_stage(int t, int n_stages) { return t < n_stages - 1 ? t : n_stages - 1; }

constexpr int64_t mf_blocks(int64_t M) { return (M + MF_CANDS - 1) / MF_CANDS; }

// LDS doubles: the B fragments of two stages [2][4 k-steps][4 fragments][64], the candidates' image [DP][32] (the fidelity column
// zero), two stages of train points [2][16][DP + 2] (the fidelity column zero), their fidelity coordinates and alphas [2][2][16].
// Behind the walk the same memory is the score's: the waves' sums [3][8][32], the means' partials [16][32], the per-candidate
// scalars [6][32] and the samples' terms [32][65] — mf_lds_tail, which is what the narrow tiers are sized by.
constexpr int mf_lds_frags() { return 2 * (MF_BK / 4) * 4 * 64; }
constexpr int mf_lds_walk(int DP) { return mf_lds_frags() + DP * MF_CANDS + 2 * MF_BK * (DP + MF_XS_PAD) + 4 * MF_BK; }
constexpr int mf_lds_tail() { return 3 * MF_WAVES * MF_CANDS + 16 * MF_CANDS + 6 * MF_CANDS + MF_CANDS * (MF_MAX_SAMPLES + 1); }
constexpr int mf_lds_doubles(int DP) { return mf_lds_walk(DP) > mf_lds_tail() ? mf_lds_walk(DP) : mf_lds_tail(); }
constexpr int64_t mf_lds_bytes(int DP) { return (int64_t)mf_lds_doubles(DP) * 8; }

}  // namespace gpbo
