// How gpla_ei2_argbest (lookahead.hip) lays out its score kernel's LDS and its workspace, as pure functions of plain values.
//
// The product in front of the epilogue is jes.hip's (jes_product.h, jes_plan.h): J <= 64 points are NF = ceil(J / 16) column
// fragments, the waves split a stage's k-steps by jes_split(J), and the product leaves cov [64][P], P = 16 NF + 1, in LDS.  The
// epilogue keeps that tile and adds two blocks behind it:
//   G  [64][P]    the product's own tile: cov_j becomes the slope g_j in place, point j >= 1 in column j - 1, point 0 (the candidate
//                 itself) in column J — the pad column where J = 16 NF, a dead column of the last fragment otherwise
//   Q  [64][P]    q_j, the latent sd at point j after the observation, same columns
//   T  [64][PH]   t_h, the best second-step EI per node; PH = H | 1
// P and PH are odd: the 64 lanes of a wave, one candidate each, read one column from 64 different banks.
// G starts where the product's stage buffers were, so the first block is as long as the longer of the two.
#pragma once

#include "jes_plan.h"

namespace gpbo {

constexpr int LA_POINTS = 64;       // GPLA_MAX_POINTS
constexpr int LA_NODES = 32;        // GPLA_MAX_NODES
constexpr int LA_LDS_BYTES_PER_CU = 160 * 1024;      // gfx950

constexpr int la_tile_pitch(int nf) { return 16 * nf + 1; }
constexpr int la_node_pitch(int H) { return H | 1; }

// offsets in doubles of Q and T, and the kernel's dynamic LDS in doubles (its static LDS is la_static_doubles on top)
constexpr int la_q_offset(int DP, int nf) { return jes_lds_doubles(DP, nf); }
constexpr int la_t_offset(int DP, int nf) { return la_q_offset(DP, nf) + JES_ROWS * la_tile_pitch(nf); }
constexpr int la_lds_doubles(int DP, int nf, int H) { return la_t_offset(DP, nf) + JES_ROWS * la_node_pitch(H); }
// m_j | p_j of the points, z_h | omega_h of the nodes
constexpr int la_static_doubles() { return 2 * LA_POINTS + 2 * LA_NODES; }

constexpr int la_lds_bytes(int DP, int nf, int H) { return 8 * (la_lds_doubles(DP, nf, H) + la_static_doubles()); }
constexpr int la_workgroups_per_cu(int DP, int nf, int H) { return LA_LDS_BYTES_PER_CU / la_lds_bytes(DP, nf, H); }

// J = 64, H = 32: 4160 + 4160 + 2112 + 192 doubles = 84992 bytes up to 32 padded dimensions (the stage buffers are shorter than the
// tile; at 64 they are 64 doubles longer: 85504), ONE workgroup per compute unit: the tile and its twin alone are 66560 bytes.
// J = 64, H = 16: 76800 bytes, two.
static_assert(la_lds_bytes(64, 4, 32) == 85504 && la_lds_bytes(32, 4, 32) == 84992 && la_lds_bytes(4, 4, 32) == 84992,
              "the budget the header states");
static_assert(la_workgroups_per_cu(64, 4, 32) == 1 && la_workgroups_per_cu(16, 4, 16) == 2, "the budget the header states");
static_assert(la_workgroups_per_cu(16, 2, 8) == 3 && la_workgroups_per_cu(16, 1, 8) == 4, "J = 32 and J = 16 at H = 8, d = 16");

// The call's workspace (ctx->la), offsets in doubles: jes_block's layout with the points in the samples' place (fraw unused), then
//   nodes [32] | weights [32]
struct LaBlock {
  JesBlock points;
  int64_t nodes, weights, doubles;
};
constexpr LaBlock la_block(int64_t J, int64_t d, int64_t DP, int64_t N, int64_t NP) {
  LaBlock b{};
  b.points = jes_block(J, d, DP, N, NP);
  b.nodes = jes_round_up(b.points.doubles, 2);
  b.weights = b.nodes + LA_NODES;
  b.doubles = b.weights + LA_NODES;
  return b;
}

}  // namespace gpbo
