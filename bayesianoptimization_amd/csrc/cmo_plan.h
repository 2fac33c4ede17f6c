// How gpmo_cnhvi_greedy lays out its workspace, as a pure function of plain values (qnehvi.hip takes every pointer from cmo_block; the
// score kernel's thread rule and LDS stage are qnehvi_plan.h's, the fronts' array size too).  Free of HIP:
// tests/test_cmo_plan_host.py compiles it with the system C++ compiler and checks that no two regions overlap, that every region
// is aligned, and that the sizes include/gpmo.h states are the ones below.
#pragma once

#include <cstdint>

#include "qnehvi_plan.h"   // QNEHVI_FRONT, qnei_even

namespace gpbo {

// The workspace (in ctx->greedy), offsets in doubles from its start, every part at an even offset (the blocks, the fronts and the
// scaled base points are read 16 bytes at a time); objective j = slot j, constraint j = slot 2 + j; T = G S draws, M candidates,
// B = n_base base points:
//   vals [2][T][M]        what the score kernel streams, objective-major: objective 0's MASKED draws (f, -inf where the draw's
//                         constraint draws call the candidate infeasible, NaN kept), objective 1's raw draws — 16 T M bytes
//   basev [2][T][ldb]     the same at the base points, ldb = B
//   front [T][L][2]       the live fronts | front0: as they were before the first pick
//   size [T] | size0 [T]  INTS: the fronts' sizes, live | before the first pick
//   viol [S][M]           ONE group's violations over the candidates: written by constraint 0, added to by the later ones, read by
//                         objective 0's pass of that group; the next group overwrites it
//   violb [S][B]          the same at the base points
//   stage [S][M]          only with values_out: one (slot, group)'s raw values on their way to the host
//   stageb [S][B]         only with base_values_out: the same at the base points
//   base (B, d)           the base points as given | base_s [B][DP] scaled by the CURRENT slot's length scales, zero padded
//   rec [q]               one record {gain, index, feasible} per pick: 3 doubles each (the index an int64)
//   flag                  ONE INT in a slot of two doubles: 0, or T - t for the lowest draw t whose front outgrew L
//   mask [M] BYTES        1 = picked in an earlier step
struct CmoBlock {
  int64_t vals, basev, front, front0, size, size0, viol, violb, stage, stageb, base, base_s, rec, flag, mask;
  int64_t ldb;
  int64_t doubles;
};
inline CmoBlock cmo_block(int T_, int S_, int64_t M, int B_, int d_, int DP_, int q_, bool values, bool base_values) {
  const int64_t T = T_, S = S_, B = B_, d = d_, DP = DP_, q = q_, L = QNEHVI_FRONT;
  CmoBlock b{};
  b.ldb = B;
  b.vals = 0;
  b.basev = qnei_even(b.vals + 2 * T * M);
  b.front = qnei_even(b.basev + 2 * T * b.ldb);
  b.front0 = b.front + T * L * 2;
  b.size = b.front0 + T * L * 2;
  b.size0 = qnei_even(b.size + (T + 1) / 2);
  b.viol = qnei_even(b.size0 + (T + 1) / 2);
  b.violb = qnei_even(b.viol + S * M);
  b.stage = qnei_even(b.violb + S * B);
  b.stageb = qnei_even(b.stage + (values ? S * M : 0));
  b.base = qnei_even(b.stageb + (base_values ? S * B : 0));
  b.base_s = qnei_even(b.base + B * d);
  b.rec = qnei_even(b.base_s + B * DP);
  b.flag = qnei_even(b.rec + 3 * q);
  b.mask = b.flag + 2;
  b.doubles = b.mask + (M + 7) / 8;
  return b;
}

}  // namespace gpbo
