// How gpje_jes_argbest (jes.hip) splits its covariance product over a workgroup and lays out its workspace, as pure functions of
// plain values.
//
// The score kernel's workgroup is four waves over JES_ROWS = 64 candidates, and S <= 64 samples are NF = ceil(S / 16) column
// fragments of v_mfma_f64_16x16x4_f64's B operand.  With one fragment per wave (ivr_plan.h's rule) S = 16 would leave three waves
// multiplying zero columns, so the waves that have no fragment of their own share one and split a stage's 8 k-steps instead:
//   jes_split(S) = 4 for NF = 1, 2 for NF = 2, 1 for NF = 3 or 4
// Wave w works on fragment u = w / split (idle in the product when u >= NF: S <= 48 at split 1) and on the k-steps
// [p 8 / split, (p + 1) 8 / split) of every stage, p = w mod split.  No zero fragment is ever multiplied; the last fragment has at
// most 15 zero columns.
//
// V = -K'^-1 k*(x*_s) is kept FRAGMENT-PACKED by (stage, fragment, k-step): the double that lane l feeds the matrix core as its B
// operand for fragment u of k-step ks of stage g sits at
//   (((g NF + u) 8 + ks) 64 + l,        train point 32 g + 4 ks + (l >> 4), sample 16 u + (l & 15)
// so the k-steps a wave owns are adjacent whatever the split, and each of its loads is one contiguous 512-byte line.
#pragma once

#include <cstdint>

namespace gpbo {

constexpr int JES_ROWS = 64;        // candidates per workgroup
constexpr int JES_KC = 32;          // train points per LDS stage (8 per wave to generate, 8 k-steps to multiply)
constexpr int JES_PITCH = 68;       // row pitch of the k-major k* block in LDS (ivr_plan.h's)
constexpr int JES_STAR = 64;        // rows of the samples' blocks (GPJE_MAX_SAMPLES), zero from S on

constexpr int jes_frags(int S) { return (S + 15) / 16; }
constexpr int jes_split(int S) { return S <= 16 ? 4 : (S <= 32 ? 2 : 1); }

constexpr int64_t jes_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// where (train point i, sample s) of V sits in the packed image
constexpr int64_t jes_packed_index(int64_t i, int64_t s, int nf) {
  const int64_t g = i / JES_KC, ks = (i % JES_KC) / 4, lane = (i % 4) * 16 + s % 16;
  return (((g * nf + s / 16) * 8) + ks) * 64 + lane;
}

// LDS doubles of the score kernel: the stage's points and its k* block, reused behind the product for the [64][16 NF + 1] sums
constexpr int jes_lds_doubles(int DP, int nf) {
  const int stage = JES_KC * DP + JES_KC * JES_PITCH, sums = JES_ROWS * (16 * nf + 1);
  return stage > sums ? stage : sums;
}

// The call's workspace (ctx->je), offsets in doubles:
//   raw (S, d) | fraw (S) | As [64][DP] | star [5][64]: m, p, rho, g, fn | zero [max(S N, NP)] | KS [S][NP] | T [S][NP] | V [S][NP] | Vp
struct JesBlock {
  int nf, split;
  int64_t Kp;
  int64_t raw, fraw, As, star, zero, n_zero, KS, T, V, Vp, n_Vp, doubles;
};
constexpr JesBlock jes_block(int64_t S, int64_t d, int64_t DP, int64_t N, int64_t NP) {
  JesBlock b{};
  b.nf = jes_frags((int)S);
  b.split = jes_split((int)S);
  b.Kp = jes_round_up(N, JES_KC);
  b.raw = 0;
  b.fraw = jes_round_up(S * d, 2);
  b.As = b.fraw + JES_STAR;
  b.star = b.As + JES_STAR * DP;
  b.zero = b.star + 5 * JES_STAR;
  b.n_zero = S * N > NP ? S * N : NP;
  b.KS = b.zero + jes_round_up(b.n_zero, 2);
  b.T = b.KS + S * NP;
  b.V = b.T + S * NP;
  b.Vp = b.V + S * NP;
  b.n_Vp = b.Kp * 16 * b.nf;
  b.doubles = b.Vp + b.n_Vp;
  return b;
}

}  // namespace gpbo
