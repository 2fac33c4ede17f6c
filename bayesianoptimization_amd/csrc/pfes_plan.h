// How gppf_pfes_argbest (pfes.hip) splits its work, stages its fronts and lays out its workspace, as pure functions of plain values.
// Free of HIP.
//
// The score kernel: lane = candidate.  A workgroup of PFES_WAVES waves serves PFES_CANDS = 64 candidates, ALL its waves the same 64:
// the draws of a staged batch are dealt over the waves, wave w taking the draws s with s mod PFES_WAVES == w, so a launch over few
// candidates still has every SIMD of a compute unit at work, and S = 1 is one wave's job.  Workgroup b serves candidates
// [64 b, 64 b + 64).
#pragma once

#include <cstdint>

#include "gppf.h"

namespace gpbo {

constexpr int PFES_CANDS = 64;                       // candidates of a workgroup: one per lane
constexpr int PFES_WAVES = 4;                        // waves of a workgroup; draw s of a batch goes to wave s mod 4
constexpr int PFES_THREADS = PFES_CANDS * PFES_WAVES;
constexpr int PFES_FRONT = GPPF_MAX_FRONT;           // L: points of one draw's front
constexpr int PFES_BATCH = 16;                       // draws whose fronts one LDS stage carries (qnehvi_plan.h: QNEHVI_CHUNK)
static_assert(PFES_BATCH % PFES_WAVES == 0, "a batch starts at a draw that is a multiple of the wave count: s mod 4 is the wave");

inline int64_t pfes_blocks(int64_t M) { return (M + PFES_CANDS - 1) / PFES_CANDS; }
inline int pfes_batches(int S) { return (S + PFES_BATCH - 1) / PFES_BATCH; }

// LDS of a workgroup, in bytes, for S draws:
//   stage [min(S, 16)][L] (a_k, c_k)      16 bytes a point, a draw owns a fixed row of L points; a wave reads a point as ONE 16-byte
//                                         broadcast (the address is the same in every lane)
//   terms [S][64]                         a_s of candidate `lane`, written by the wave that has draw s, summed s = 0 .. S - 1 by wave 0
// The limit, S = 64: 16 x 128 x 16 + 64 x 64 x 8 = 32768 + 32768 = 65536 bytes — what a workgroup gets without asking, and two
// workgroups (8 waves, two per SIMD) in a compute unit's 160 KiB.  S = 16: 32768 + 8192 = 40960 bytes, four workgroups (16 waves).
constexpr int64_t PFES_CU_LDS_BYTES = 160 * 1024;
inline int64_t pfes_stage_bytes(int S) { return (int64_t)(S < PFES_BATCH ? S : PFES_BATCH) * PFES_FRONT * 16; }
inline int64_t pfes_lds_bytes(int S) { return pfes_stage_bytes(S) + (int64_t)S * PFES_CANDS * 8; }
inline int pfes_blocks_per_cu(int S) { return (int)(PFES_CU_LDS_BYTES / pfes_lds_bytes(S)); }
constexpr int64_t PFES_MAX_LDS_BYTES = (int64_t)PFES_BATCH * PFES_FRONT * 16 + (int64_t)GPPF_MAX_SAMPLES * PFES_CANDS * 8;
static_assert(PFES_MAX_LDS_BYTES <= 64 * 1024, "the largest instance stays inside the 64 KiB a workgroup gets without asking");
static_assert(2 * PFES_MAX_LDS_BYTES <= PFES_CU_LDS_BYTES, "two workgroups of the largest instance share a compute unit's 160 KiB");

// The workspace (ctx->pf), offsets in doubles from its start, every part at an even offset; S draws, B = the candidates the draws
// are evaluated at in device-front mode (0 in host-front mode):
//   vals [2][S][B]        the joint draws' values, objective-major
//   front [S][L][2]       the fronts the score kernel reads | front0: qnehvi_front_kernel's second copy (not read)
//   size [S] | size0 [S]  INTS: the fronts' sizes
//   flag                  ONE INT in a slot of two doubles: 0, or S - s for the lowest draw s whose front outgrew L
struct PfesBlock {
  int64_t vals, front, front0, size, size0, flag;
  int64_t doubles;
};
inline int64_t pfes_even(int64_t x) { return (x + 1) & ~(int64_t)1; }
inline PfesBlock pfes_block(int S_, int64_t B) {
  const int64_t S = S_, L = PFES_FRONT;
  PfesBlock b{};
  b.vals = 0;
  b.front = pfes_even(b.vals + 2 * S * B);
  b.front0 = b.front + S * L * 2;
  b.size = b.front0 + S * L * 2;
  b.size0 = pfes_even(b.size + (S + 1) / 2);
  b.flag = pfes_even(b.size0 + (S + 1) / 2);
  b.doubles = b.flag + 2;
  return b;
}

}  // namespace gpbo
