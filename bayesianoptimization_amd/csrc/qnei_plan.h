// How gpbo_qnei_greedy lays out its workspace and dispatches its score kernel, as pure functions of plain values (qnei.hip takes
// every pointer from qnei_block and every launch shape from the rules below).  Free of HIP: tests/test_qnei_plan_host.py compiles it
// with the system C++ compiler and pins every offset and both sides of every edge.
#pragma once

#include <cstdint>

#include "gpbo.h"   // GPBO_MAX_PATHS, GPBO_MAX_QNEI_GROUPS, GPBO_MAX_QNEI_POINTS, GPBO_MAX_SEEDS

namespace gpbo {

constexpr int QNEI_BLOCK = 256;                                        // threads of a qnei_score_kernel workgroup
constexpr int QNEI_MAX_DRAWS = GPBO_MAX_QNEI_GROUPS * GPBO_MAX_PATHS;   // T <= 256: the incumbents fit one LDS array of 2 KiB

// Candidates a thread of qnei_score_kernel serves.  The kernel is a stream of the T rows of the block, rows M doubles apart: with M
// even every row starts on a 16-byte boundary and a thread reads two neighbouring candidates as ONE 16-byte load (the width at
// which a wave's load is 1 KiB and the memory pipe runs at its full rate); with M odd every other row starts 8 bytes off, a 16-byte
// load would be misaligned, and a thread serves one candidate with 8-byte loads (a wave still reads 512 contiguous bytes).  The
// arithmetic of a candidate is the same either way.
inline int qnei_items(int64_t M) { return M % 2 == 0 ? 2 : 1; }
// ... the first of them: thread `thread` of workgroup `block` serves candidates [first, first + items) that are < M (constexpr: the
// kernel calls it too)
constexpr int64_t qnei_first_candidate(int64_t block, int thread, int items) { return (block * QNEI_BLOCK + thread) * items; }
inline int64_t qnei_score_blocks(int64_t M) {
  const int64_t per_block = (int64_t)QNEI_BLOCK * qnei_items(M);
  return (M + per_block - 1) / per_block;
}

// The workspace (in ctx->greedy), offsets in doubles from its start, every part at an even offset (the block is read as double2, the
// scaled pending points too):
//   vals [T][M]      the draws' values over the candidates, row t = g S + s: 8 T M bytes — 2 GiB at T = 256, M = 2^20
//   base [T][ldb]    the draws' values at the N training points | the P pending points, ldb = N + P
//   m [T] | m0 [T]   the incumbents (updated between the picks) | as they were before the first pick (baseline_out)
//   pend (P, d)      the pending points as given | pend_s [P][DP] scaled by the slot's length scales, zero padded
//   rec [q]          one record {gain, index} per pick: 2 doubles each (the index an int64)
//   mask [M] BYTES   1 = picked in an earlier step
struct QneiBlock {
  int64_t vals, base, m, m0, pend, pend_s, rec, mask;
  int64_t ldb;
  int64_t doubles;
};
inline int64_t qnei_even(int64_t x) { return (x + 1) / 2 * 2; }
inline QneiBlock qnei_block(int T_, int64_t M, int N_, int P_, int d_, int DP_, int q_) {
  const int64_t T = T_, N = N_, P = P_, d = d_, DP = DP_, q = q_;
  QneiBlock b{};
  b.ldb = N + P;
  b.vals = 0;
  b.base = qnei_even(b.vals + T * M);
  b.m = qnei_even(b.base + T * b.ldb);
  b.m0 = qnei_even(b.m + T);
  b.pend = qnei_even(b.m0 + T);
  b.pend_s = qnei_even(b.pend + P * d);
  b.rec = qnei_even(b.pend_s + P * DP);
  b.mask = b.rec + 2 * q;
  b.doubles = b.mask + (M + 7) / 8;
  return b;
}

}  // namespace gpbo
