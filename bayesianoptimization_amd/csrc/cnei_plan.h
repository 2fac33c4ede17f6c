// How gpbo_cnei_greedy lays out its workspace, as a pure function of plain values (qnei.hip takes every pointer from cnei_block; the
// score kernel's thread rule is qnei_plan.h's).  Free of HIP: tests/test_cnei_plan_host.py compiles it with the system C++ compiler
// and pins every offset and both sides of every edge.
#pragma once

#include <cstdint>

namespace gpbo {

// The workspace (in ctx->greedy), offsets in doubles from its start, every part at an even offset (the block and the scaled base points
// are read as double2).  T = G S draws, M candidates, B = n_base base points:
//   vals [T][M]        the MASKED objective draws over the candidates, row t = g S + s: f, -inf where the draw calls the
//                      candidate infeasible, NaN kept — 8 T M bytes, the block the score kernel streams
//   base [T][B]        the masked objective draws at the base points (ldb = B)
//   m [T] | m0 [T]     the incumbents (updated between the picks) | as they were before the first pick (baseline_out)
//   viol [S][M]        ONE group's violations over the candidates: written by constraint 1, added to by the later ones, read by the
//                      objective's pass of that group; the next group overwrites it
//   violb [S][B]       the same at the base points
//   stage [S][M]       only with values_out: one (slot, group)'s raw values on their way to the host
//   stageb [S][B]      only with base_values_out: the same at the base points
//   pts (B, d)         the base points as given | pts_s [B][DP] scaled by the CURRENT slot's length scales, zero padded
//   rec [q]            one record {gain, index, feasible} per pick: 3 doubles each (the index an int64)
//   mask [M] BYTES     1 = picked in an earlier step
struct CneiBlock {
  int64_t vals, base, m, m0, viol, violb, stage, stageb, pts, pts_s, rec, mask;
  int64_t ldb;
  int64_t doubles;
};
inline int64_t cnei_even(int64_t x) { return (x + 1) / 2 * 2; }
inline CneiBlock cnei_block(int T_, int S_, int64_t M, int B_, int d_, int DP_, int q_, bool values, bool base_values) {
  const int64_t T = T_, S = S_, B = B_, d = d_, DP = DP_, q = q_;
  CneiBlock b{};
  b.ldb = B;
  b.vals = 0;
  b.base = cnei_even(b.vals + T * M);
  b.m = cnei_even(b.base + T * B);
  b.m0 = cnei_even(b.m + T);
  b.viol = cnei_even(b.m0 + T);
  b.violb = cnei_even(b.viol + S * M);
  b.stage = cnei_even(b.violb + S * B);
  b.stageb = cnei_even(b.stage + (values ? S * M : 0));
  b.pts = cnei_even(b.stageb + (base_values ? S * B : 0));
  b.pts_s = cnei_even(b.pts + B * d);
  b.rec = cnei_even(b.pts_s + B * DP);
  b.mask = cnei_even(b.rec + 3 * q);
  b.doubles = b.mask + (M + 7) / 8;
  return b;
}

}  // namespace gpbo
