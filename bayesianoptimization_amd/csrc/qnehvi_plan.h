// How gpbo_qnhvi_greedy lays out its workspace and dispatches its score kernel, as pure functions of plain values (qnehvi.hip takes
// every pointer from qnehvi_block and every launch shape from the rules below and from qnei_plan.h's).  Free of HIP:
// tests/test_qnehvi_plan_host.py compiles it with the system C++ compiler and pins every offset and both sides of every edge.
#pragma once

#include <cstdint>

#include "gpbo.h"        // GPBO_MAX_QNEHVI_FRONT, GPBO_MAX_QNEHVI_BASE
#include "qnei_plan.h"   // QNEI_BLOCK, QNEI_MAX_DRAWS, qnei_items / qnei_first_candidate / qnei_score_blocks / qnei_even

namespace gpbo {

constexpr int QNEHVI_FRONT = GPBO_MAX_QNEHVI_FRONT;      // L: points of one draw's front
constexpr int QNEHVI_STRIPS = QNEHVI_FRONT + 1;          // strips k = 0 .. n of a front of n <= L points

// The score kernel's thread rule is qnei_score_kernel's: qnei_items(M) neighbouring candidates per thread (two with one 16-byte load
// per row where M is even — both objectives' (T, M) blocks then start on a 16-byte boundary, 8 T M bytes apart —, one with 8-byte
// loads where M is odd), thread `thread` of workgroup `block` serving qnei_first_candidate(block, thread, items) onwards, in
// qnei_score_blocks(M) workgroups of QNEI_BLOCK threads.

// Draws whose fronts ONE LDS stage of the score kernel carries.  A strip is 16 bytes, (a_{k+1}, c_k), and a draw owns a fixed slot
// of QNEHVI_STRIPS strips (its front's size is known on the device only, and nothing waits for it): 2064 bytes a draw.  16 draws are
// 33,024 bytes — four workgroups (16 waves) share a CU's 160 KiB, enough to hide the stream's latency; T <= 16 stages once.
constexpr int QNEHVI_CHUNK = 16;
inline int qnehvi_chunk_draws(int T) { return T < QNEHVI_CHUNK ? T : QNEHVI_CHUNK; }
inline int qnehvi_chunks(int T) { return (T + QNEHVI_CHUNK - 1) / QNEHVI_CHUNK; }
constexpr int64_t QNEHVI_LDS_BYTES = (int64_t)QNEHVI_CHUNK * QNEHVI_STRIPS * 16 + QNEHVI_CHUNK * 4;

// The workspace (in ctx->greedy), offsets in doubles from its start, every part at an even offset (the blocks and the fronts are read
// 16 bytes at a time); objective j = slot j, T draws, M candidates, B = n_base:
//   vals [2][T][M]        the draws' values over the candidates, objective-major: 16 T M bytes — 4 GiB at T = 256, M = 2^20
//   basev [2][T][ldb]     the draws' values at the B base points, ldb = B
//   front [T][L][2]       the live fronts, point k of draw t = (a, c) | front0: as they were before the first pick
//   size [T] | size0 [T]  INTS: the fronts' sizes, live | before the first pick
//   base (B, d)           the base points as given | base_s [2][B][DP] scaled by slot j's length scales, zero padded
//   rec [q]               one record {gain, index} per pick: 2 doubles each (the index an int64)
//   flag                  ONE INT in a slot of two doubles: 0, or T - t for the lowest draw t whose front outgrew L
//   mask [M] BYTES        1 = picked in an earlier step
struct QnehviBlock {
  int64_t vals, basev, front, front0, size, size0, base, base_s, rec, flag, mask;
  int64_t ldb;
  int64_t doubles;
};
inline QnehviBlock qnehvi_block(int T_, int64_t M, int B_, int d_, int DP_, int q_) {
  const int64_t T = T_, B = B_, d = d_, DP = DP_, q = q_, L = QNEHVI_FRONT;
  QnehviBlock b{};
  b.ldb = B;
  b.vals = 0;
  b.basev = qnei_even(b.vals + 2 * T * M);
  b.front = qnei_even(b.basev + 2 * T * b.ldb);
  b.front0 = b.front + T * L * 2;
  b.size = b.front0 + T * L * 2;
  b.size0 = qnei_even(b.size + (T + 1) / 2);
  b.base = qnei_even(b.size0 + (T + 1) / 2);
  b.base_s = qnei_even(b.base + B * d);
  b.rec = qnei_even(b.base_s + 2 * B * DP);
  b.flag = b.rec + 2 * q;
  b.mask = b.flag + 2;
  b.doubles = b.mask + (M + 7) / 8;
  return b;
}

}  // namespace gpbo
