// How gpmo3_nhvi_greedy lays out its workspace and packs the LDS stages of its score kernel, as pure functions of plain values
// (qnehvi3.hip takes every pointer from qnehvi3_block and every stage boundary from qnehvi3_stage_draws; the thread rule is
// qnei_plan.h's).  Free of HIP: tests/test_qnehvi3_host.py compiles it with the system C++ compiler and pins every offset, the
// packing rule and both sides of the budget edge.
#pragma once

#include <cstdint>

#include "gpbo.h"        // GPBO_MAX_QNEHVI_FRONT, GPBO_MAX_QNEHVI_BASE
#include "qnei_plan.h"   // QNEI_BLOCK, QNEI_MAX_DRAWS, qnei_items / qnei_first_candidate / qnei_score_blocks / qnei_even

namespace gpbo {

constexpr int QNEHVI3_FRONT = GPBO_MAX_QNEHVI_FRONT;      // L: points of one draw's front
constexpr int QNEHVI3_CELLS = 2 * QNEHVI3_FRONT + 1;      // cells of a front of L points: the height-map sweep emits at most 2 n + 1
constexpr int QNEHVI3_CELL = 5;                           // doubles of a cell: x_lo, x_hi, y_lo, y_hi, h
constexpr int QNEHVI3_WAVE = 64;                          // threads of the update kernel's workgroup: one wave per draw

// One LDS stage of the score kernel.  A cell is 40 bytes and a draw has 1 .. QNEHVI3_CELLS of them — typically a few dozen —, so a
// stage is packed by the draws' ACTUAL cell counts: from draw t0 on it takes draws while their cells together stay within
// QNEHVI3_STAGE_CELLS and their number within QNEHVI3_STAGE_DRAWS.  One draw always fits (QNEHVI3_CELLS <= QNEHVI3_STAGE_CELLS), so
// every stage advances.  The counts lie in global memory and are the same for every thread: the boundaries are uniform.  In LDS a
// stage is three planes — (x_lo, x_hi) and (y_lo, y_hi) as 16-byte pairs, h as 8 bytes — and the draws' first cells:
// 40 * 1008 + 4 * 64 = 40,576 bytes, so four workgroups (16 waves) share a CU's 160 KiB.
constexpr int QNEHVI3_STAGE_CELLS = 1008;
constexpr int QNEHVI3_STAGE_DRAWS = 63;
constexpr int64_t QNEHVI3_LDS_BYTES = (int64_t)QNEHVI3_STAGE_CELLS * QNEHVI3_CELL * 8 + (QNEHVI3_STAGE_DRAWS + 1) * 4;
static_assert(QNEHVI3_CELLS <= QNEHVI3_STAGE_CELLS, "a stage holds at least one draw");
static_assert(4 * QNEHVI3_LDS_BYTES <= 160 * 1024, "four workgroups share a CU's LDS");

// a draw's cell count as the kernels read it: never outside its array
constexpr int qnehvi3_count(int n) { return n < 0 ? 0 : (n > QNEHVI3_CELLS ? QNEHVI3_CELLS : n); }
// Draws of the stage that starts at draw t0 < T (>= 1); *cells: their cells together (constexpr: the kernel calls it too)
constexpr int qnehvi3_stage_draws(const int* counts, int t0, int T, int* cells) {
  int total = qnehvi3_count(counts[t0]), n = 1;
  while (t0 + n < T && n < QNEHVI3_STAGE_DRAWS && total + qnehvi3_count(counts[t0 + n]) <= QNEHVI3_STAGE_CELLS)
    total += qnehvi3_count(counts[t0 + n++]);
  *cells = total;
  return n;
}

// The workspace (in ctx->greedy), offsets in doubles from its start, every part at an even offset (the blocks are read 16 bytes at a
// time); objective j = slot j, T draws, M candidates, B = n_base, L = QNEHVI3_FRONT, C = QNEHVI3_CELLS:
//   vals [3][T][M]          the draws' values over the candidates, objective-major: 24 T M bytes — 6 GiB at T = 256, M = 2^20
//   basev [3][T][ldb]       the draws' values at the B base points, ldb = B
//   front [T][L][3]         the live fronts in stored order (objective 2, then 0, then 1, all descending) | front0: before the first pick
//   cells [T][C][5]         the live cells in emission order | cells0: before the first pick
//   size, size0 [T] INTS    the fronts' sizes, live | before the first pick;  ncell, ncell0 [T] INTS: the cell counts
//   base (B, d)             the base points as given | base_s [3][B][DP] scaled by slot j's length scales, zero padded
//   rec [q]                 one record {gain, index} per pick: 2 doubles each (the index an int64)
//   flag                    ONE INT in a slot of two doubles: 0, or T - t for the lowest draw t whose front outgrew L
//   mask [M] BYTES          1 = picked in an earlier step
struct Qnehvi3Block {
  int64_t vals, basev, front, front0, cells, cells0, size, size0, ncell, ncell0, base, base_s, rec, flag, mask;
  int64_t ldb;
  int64_t doubles;
};
inline Qnehvi3Block qnehvi3_block(int T_, int64_t M, int B_, int d_, int DP_, int q_) {
  const int64_t T = T_, B = B_, d = d_, DP = DP_, q = q_, L = QNEHVI3_FRONT, C = QNEHVI3_CELLS;
  const int64_t ints = qnei_even((T + 1) / 2);
  Qnehvi3Block b{};
  b.ldb = B;
  b.vals = 0;
  b.basev = qnei_even(b.vals + 3 * T * M);
  b.front = qnei_even(b.basev + 3 * T * b.ldb);
  b.front0 = b.front + T * L * 3;
  b.cells = b.front0 + T * L * 3;
  b.cells0 = qnei_even(b.cells + T * C * QNEHVI3_CELL);
  b.size = qnei_even(b.cells0 + T * C * QNEHVI3_CELL);
  b.size0 = b.size + ints;
  b.ncell = b.size0 + ints;
  b.ncell0 = b.ncell + ints;
  b.base = b.ncell0 + ints;
  b.base_s = qnei_even(b.base + B * d);
  b.rec = qnei_even(b.base_s + 3 * B * DP);
  b.flag = b.rec + 2 * q;
  b.mask = b.flag + 2;
  b.doubles = b.mask + (M + 7) / 8;
  return b;
}

}  // namespace gpbo
