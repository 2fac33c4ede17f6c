// How gpls_sur_argbest (sur.hip) lays out its workspace and the quadrature rule of its epilogue, as pure functions of plain values.
//
// The product is gpiv_ivr_argbest's: the same column tiles (ivr_plan.h: 64 * NSUB integration points per tile, NSUB the narrowest of
// 1, 2, 4 whose tile holds J), the same fragment-packed V.  Behind ivr_block's layout the workspace keeps three scalars per column,
// zero from J on (a padded column has omega = 0, h2 = 0 and is2 = 0: r2 = 0, a term of exactly 0):
//   h2 [Jp] = h_j^2 | is2 [Jp] = 1 / s_j^2 (0 where s_j = 0) | p [Jp] = Phi(h_j)
#pragma once

#include "ivr_plan.h"

namespace gpbo {

// G(h2, r2) = (1 / pi) int_0^U exp(-h2 (1 + u^2) / (1 + u)^2) / (1 + u^2) du by Gauss-Legendre on [0, U]: the nodes and weights of
// the rule on [0, 1], ascending.  12 nodes: |error| <= 2e-15 absolute over h in [0, 8] x r2 in [0, 1] (the integrand's nearest
// singularities are u = +-i and u = -1, outside the Bernstein ellipse of radius 4.6 around [0, 1]); 8 nodes leave 7e-11.
constexpr int SUR_NODES = 12;
constexpr double SUR_NODE_X[SUR_NODES] = {0.0092196828766403746547, 0.047941371814762571661, 0.11504866290284765648,
                                          0.20634102285669127635,   0.31608425050090990312,  0.43738329574426554226,
                                          0.56261670425573445774,   0.68391574949909009688,  0.79365897714330872365,
                                          0.88495133709715234352,   0.95205862818523742834,  0.99078031712335962535};
constexpr double SUR_NODE_W[SUR_NODES] = {0.023587668193255913597, 0.05346966299765921548, 0.080039164271673113167,
                                          0.10158371336153296087,  0.11674626826917740438, 0.1245735229067013925,
                                          0.1245735229067013925,   0.11674626826917740438, 0.10158371336153296087,
                                          0.080039164271673113167, 0.05346966299765921548, 0.023587668193255913597};

// The call's workspace (ctx->ls), offsets in doubles: ivr_block's layout | h2 [Jp] | is2 [Jp] | p [Jp]
struct SurBlock {
  IvrBlock iv;
  int64_t h2, is2, p, doubles;
};
constexpr SurBlock sur_block(int64_t J, int64_t d, int64_t DP, int64_t N, int64_t NP) {
  SurBlock b{};
  b.iv = ivr_block(J, d, DP, N, NP);
  b.h2 = ivr_round_up(b.iv.doubles, 2);
  b.is2 = b.h2 + b.iv.Jp;
  b.p = b.is2 + b.iv.Jp;
  b.doubles = b.p + b.iv.Jp;
  return b;
}

}  // namespace gpbo
