// How gpnn_acq_argbest (nngp.hip) splits its work and lays out its LDS and its workspace, as pure functions of plain values.
//
// Search (nn_search_kernel).  Lane = candidate; a workgroup owns nn_search_cands(k) of them — every wave its own 64, the waves share
// only the staged chunk of NN_CHUNK rows, so no lists are merged.  LDS per workgroup, out of the CU's 160 KB:
//   d2  [k][cands] fp64 | index [k][cands] int32      12 B per list entry, [slot][lane]: a wave's 64 lanes hit 64 consecutive words
//   rows [NN_CHUNK][DP] fp64                           the staged chunk, read as broadcasts
//   k = 64: 128 candidates, 96 KB of lists; k = 32: 256, 96 KB; k = 16: 256, 48 KB; the chunk adds 1 KB (DP = 4) .. 16 KB (DP = 64).
// Solve (nn_solve_kernel).  One wave owns 64 / k candidates, lane = (candidate, row).  LDS per wave:
//   A    [64 / k][k][k + 1] fp64                       the lower triangles; the pitch k + 1 spreads a column over the banks
//   row  [2][64 / k][DP] fp64                          the neighbour row being broadcast, double-buffered
//   k = 64: 33 280 B + 16 DP; four waves per workgroup hold 133 KB + 4 KB at DP = 64.
#pragma once

#include <cstdint>

namespace gpbo {

constexpr int NN_CHUNK = 32;            // rows per staged chunk of the search
constexpr int NN_SOLVE_WAVES = 4;       // waves per workgroup of the solve
constexpr int NN_LDS_BYTES = 160 * 1024;

constexpr bool nn_k_ok(int k) { return k == 16 || k == 32 || k == 64; }
// candidates (= threads) per workgroup of the search
constexpr int nn_search_cands(int k) { return k == 64 ? 128 : 256; }
constexpr int64_t nn_search_lds(int k, int DP) {
  return (int64_t)k * nn_search_cands(k) * 12 + (int64_t)NN_CHUNK * DP * 8;
}
// candidates per wave / per workgroup of the solve
constexpr int nn_solve_pack(int k) { return 64 / k; }
constexpr int nn_solve_cands(int k) { return NN_SOLVE_WAVES * nn_solve_pack(k); }
constexpr int64_t nn_solve_lds(int k, int DP) {
  return (int64_t)NN_SOLVE_WAVES * nn_solve_pack(k) * ((int64_t)k * (k + 1) + 2 * DP) * 8;
}
static_assert(nn_search_lds(64, 64) <= NN_LDS_BYTES && nn_search_lds(32, 64) <= NN_LDS_BYTES && nn_search_lds(16, 64) <= NN_LDS_BYTES,
              "the search's lists and chunk fit the LDS");
static_assert(nn_solve_lds(64, 64) <= NN_LDS_BYTES && nn_solve_lds(32, 64) <= NN_LDS_BYTES && nn_solve_lds(16, 64) <= NN_LDS_BYTES,
              "the solve's triangles fit the LDS");

constexpr int64_t nn_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// The call's workspace (ctx->nn), offsets in doubles:
//   ls [64] | raw [N d] the rows as given | y [N] | Xs [Np][DP] the scaled rows, zero rows from N on | Ps [Mp][DP] the scaled
//   candidates | mu [M] | sd [M] | nbr [M k] int32, two per double
// Np covers the search's last chunk, which starts at a row k + 32 c: below N + 32.  Mp covers a workgroup's repeat of row M - 1.
struct NnBlock {
  int64_t Np, Mp;
  int64_t ls, raw, y, Xs, Ps, mu, sd, nbr, doubles;
};
constexpr NnBlock nn_block(int64_t N, int64_t d, int64_t DP, int64_t M, int64_t k) {
  NnBlock b{};
  b.Np = nn_round_up(N, NN_CHUNK) + NN_CHUNK;
  b.Mp = nn_round_up(M, 256);
  b.ls = 0;
  b.raw = 64;
  b.y = nn_round_up(b.raw + N * d, 2);
  b.Xs = nn_round_up(b.y + N, 2);
  b.Ps = b.Xs + b.Np * DP;
  b.mu = b.Ps + b.Mp * DP;
  b.sd = b.mu + M;
  b.nbr = nn_round_up(b.sd + M, 2);
  b.doubles = b.nbr + (M * k + 1) / 2;
  return b;
}

}  // namespace gpbo
