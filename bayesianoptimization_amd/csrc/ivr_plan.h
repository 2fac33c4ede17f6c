// How gpiv_ivr_argbest (ivr.hip) tiles its covariance product and lays out its workspace, as pure functions of plain values.
//
// The score kernel's workgroup is four waves over IVR_ROWS = 64 candidates.  A column tile is 64 * NSUB integration points: wave w
// owns the 16 * NSUB columns behind column 16 * NSUB * w of the tile, as NSUB fragments of v_mfma_f64_16x16x4_f64's B operand.
// NSUB is the dispatch rule's (ivr_nsub): the narrowest of 1, 2, 4 whose tile holds J, so that a small J multiplies few zero
// columns; J > 256 walks tiles of 256.  J is padded to whole tiles (Jp), N to whole stages of IVR_KC train points (Kp <= NP: NP is
// a multiple of 64).
//
// V = -K'^-1 k*(a_j) is kept FRAGMENT-PACKED: the double that lane l of wave w feeds the matrix core as its B operand for column
// fragment u of k-step ks (train points 4 ks .. 4 ks + 3) of tile t sits at
//   ((((t * Kp / 4) + ks) * 4 + w) * NSUB + u) * 64 + l,       train point 4 ks + (l >> 4), column 64 NSUB t + 16 NSUB w + 16 u + (l & 15)
// so a wave's load is one contiguous 512-byte line and the kernel does no address arithmetic beyond a running pointer.
#pragma once

#include <cstdint>

namespace gpbo {

constexpr int IVR_ROWS = 64;        // candidates per workgroup
constexpr int IVR_KC = 32;          // train points per LDS stage (8 per wave to generate, 8 k-steps to multiply)
constexpr int IVR_PITCH = 68;       // row pitch of the k-major k* block in LDS (gemm_tile.h's)
constexpr int IVR_GROUP = 256;      // columns per launch of the points stage (a multiple of every tile width)

// 16-column fragments per wave for J integration points
constexpr int ivr_nsub(int J) { return J <= 64 ? 1 : (J <= 128 ? 2 : 4); }
constexpr int ivr_tile_cols(int nsub) { return 64 * nsub; }

constexpr int64_t ivr_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// where (train point i, column j) of V sits in the packed image
constexpr int64_t ivr_packed_index(int64_t i, int64_t j, int nsub, int64_t Kp) {
  const int64_t cw = ivr_tile_cols(nsub), nwc = 16 * nsub;
  const int64_t tile = j / cw, within = j % cw;
  const int64_t w = within / nwc, u = (within % nwc) / 16, c = within % 16;
  const int64_t ks = i / 4, lane = (i % 4) * 16 + c;
  return ((((tile * (Kp / 4)) + ks) * 4 + w) * nsub + u) * 64 + lane;
}

// The call's workspace (ctx->iv), offsets in doubles:
//   raw (J, d) | wraw (J) | As [Jp][DP] | omega [Jp] | zero [max(G N, NP)] | KS [G][NP] | T [G][NP] | V [G][NP] | Vp [Jp][Kp]
// G = min(J, IVR_GROUP): the points stage runs in column groups, so everything but Vp stays small.  O(J NP) doubles.
struct IvrBlock {
  int nsub;
  int64_t Jp, Kp, n_tiles, G;
  int64_t raw, wraw, As, omega, zero, n_zero, KS, T, V, Vp, doubles;
};
constexpr IvrBlock ivr_block(int64_t J, int64_t d, int64_t DP, int64_t N, int64_t NP) {
  IvrBlock b{};
  b.nsub = ivr_nsub((int)J);
  b.Jp = ivr_round_up(J, ivr_tile_cols(b.nsub));
  b.Kp = ivr_round_up(N, IVR_KC);
  b.n_tiles = b.Jp / ivr_tile_cols(b.nsub);
  b.G = J < IVR_GROUP ? J : IVR_GROUP;
  b.raw = 0;
  b.wraw = ivr_round_up(J * d, 2);
  b.As = b.wraw + ivr_round_up(J, 2);
  b.omega = b.As + b.Jp * DP;
  b.zero = b.omega + b.Jp;
  b.n_zero = b.G * N > NP ? b.G * N : NP;
  b.KS = b.zero + ivr_round_up(b.n_zero, 2);
  b.T = b.KS + b.G * NP;
  b.V = b.T + b.G * NP;
  b.Vp = b.V + b.G * NP;
  b.doubles = b.Vp + b.Jp * b.Kp;
  return b;
}

}  // namespace gpbo
