// Fixed-point int8 digit planes of the posterior GEMM on int8 matrix cores (posterior_i8.hip), host and device.
//
// Scheme (Ozaki I, fixed point, balanced base-256 digits): an operand x with |x| <= 1 is rounded once to the integer
// Q = rint(x 2^(8S-2)), |Q| <= 2^(8S-2), and Q is written as S digits, Q = sum_{t=0..S-1} b_t 256^(S-1-t), with
// b_1 ... b_{S-1} in [-128, 127] and the leading b_0 in [-65, 65].  k* needs no scale (0 <= k* <= 1 for unit-amplitude
// Matern / RBF, 1.0 exact); a row i of W = L^-1 is divided by 2^e_i, e_i = frexp exponent of max_j |W_ij|.  The GEMM
// keeps the products (s, t) with s + t <= S - 1 (0-based digits) and sums the products of one level l = s + t into one
// int32 per output: exact, so the result depends on no tile shape, K order, slab or grid.  The epilogue turns the S
// level sums of one output into its fp64 value with ONE rounding (i8_combine).
//
// Digits come from Q + OFF, OFF = 128 (256^(S-2) + ... + 1): the bytes of that integer below the leading one are b_t + 128
// (t >= 1), its leading byte (arithmetic shift) is b_0; no per-digit carry.
#pragma once

#include <cmath>
#include <cstdint>

#include "posterior_plan.h"   // I8_S, the digits per operand; I8_NP_MAX, the largest NP the int8 GEMM serves

#if defined(__HIPCC__)
#define GPBO_HD __host__ __device__
#else
#define GPBO_HD
#endif

namespace gpbo {

// I8_S = 7 digits per operand: 28 int8 products, truncation ~2^-54 of max_j|W_ij| sum_j k*_j
// the int32 level sums: a level holds <= S products of |digit| <= 128 per train point
static_assert((int64_t)I8_S * 128 * 128 * I8_NP_MAX < ((int64_t)1 << 31), "int32 level sums overflow at I8_NP_MAX");

template <int S>
GPBO_HD constexpr int64_t i8_offset() {
  int64_t o = 0;
  for (int t = 1; t < S; ++t) o = o * 256 + 128;
  return o;
}

// x (|x| <= 2^(8S-2) after scaling) -> nearest integer, ties to even on host and device alike
GPBO_HD inline int64_t i8_round(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __double2ll_rn(x);
#else
  return (int64_t)std::nearbyint(x);
#endif
}

// Q + OFF of a value already scaled to |x| <= 1: k* (scale 1) or W_ij / 2^e_i
template <int S>
GPBO_HD inline int64_t i8_quantize(double x) {
  return i8_round(std::ldexp(x, 8 * S - 2)) + i8_offset<S>();
}

// byte t (0 = leading digit) of the digit planes of Qo = Q + OFF, as the int8 two's-complement byte
template <int S>
GPBO_HD inline uint32_t i8_digit_byte(int64_t Qo, int t) {
  return (uint32_t)((Qo >> (8 * (S - 1 - t))) & 255) ^ (t ? 128u : 0u);
}

// 2^e of W row i: the frexp exponent of max_j |W_ij| (|W_ij| / 2^e < 1); 0 for an all-zero row
GPBO_HD inline int i8_row_exponent(double maxabs) {
  int e = 0;
  (void)std::frexp(maxabs, &e);
  return maxabs > 0.0 ? e : 0;
}

// ---- operand layout of v_mfma_i32_16x16x64_i8 (posterior_i8.hip) ----------------------------------------------------------
// Both operands lie in fragment order, [block of 16 items][64-step][plane][lane] 16 bytes: an item is a row of W or a candidate,
// a 64-step is 64 consecutive train points, lane 16 g + r holds item r's bytes for train points 16 g ... 16 g + 15 of the step.
// Index of the 16-byte fragment that holds (item of the block, train point k, plane), given the block's first 64-step in its buffer:
template <int S>
GPBO_HD constexpr int64_t i8_frag_index(int64_t first_step, int64_t k, int plane, int item) {
  return ((first_step + (k >> 6)) * S + plane) * 64 + ((k >> 4) & 3) * 16 + item;
}
// k* digits: every block of 16 candidates holds all NP / 64 steps
GPBO_HD constexpr int64_t i8_kd_block(int64_t cb, int64_t NP) { return cb * (NP / 64); }
// W digits, lower triangle: the block of rows 16 b ... 16 b + 15 holds the steps 0 ... b / 4 (the last one zero where it lies past
// the diagonal), so it starts at sum_{b' < b} (b' / 4 + 1); no padding steps
GPBO_HD constexpr int64_t i8_wd_block(int64_t b) {
  const int64_t q = b >> 2, r = b & 3;
  return b + 2 * q * (q - 1) + r * q;
}

// The S level sums of one output (acc[l], l = s + t, weight 256^(2S-2-l) in units of 2^-(16S-4)) -> their sum in fp64, in
// units of the lowest level (times 2^i8_scale_exp(e) that is v_i).  Every level converts exactly; the levels are taken in
// three groups whose sums are exact (each spans fewer than 53 bits: the top S - 4 levels, the next two, the last two), the
// two upper groups are added with an error-free TwoSum, and the two remaining low parts are added to the rounded head:
// within 1 ulp of the exact sum of the truncated digit product.  (Integer arithmetic would make it exact, but its 64-bit
// temporaries spill the GEMM's registers in the epilogue.)
template <int S>
GPBO_HD inline double i8_combine(const int32_t* acc) {
  static_assert(S >= 5 && S <= 7, "groups of S - 4, 2 and 2 levels");
  double h = 0.0;                                           // levels 0 .. S-5, lowest bit 2^32: < 2^(31+8(S-5)+1) wide
  for (int l = 0; l < S - 4; ++l) h = h * 256.0 + (double)acc[l];
  h *= 4294967296.0;
  const double m = (double)acc[S - 4] * 16777216.0 + (double)acc[S - 3] * 65536.0;   // lowest bit 2^16, < 2^56
  const double lo = (double)acc[S - 2] * 256.0 + (double)acc[S - 1];                 // < 2^40
  const double s = h + m;                                   // TwoSum(h, m): s + e == h + m exactly
  const double bb = s - h;
  const double e = (h - (s - bb)) + (m - bb);
  return s + (e + lo);
}

// the power of two that turns i8_combine's value (units of the lowest level) into v_i for a row of exponent e
template <int S>
GPBO_HD constexpr int i8_scale_exp(int e) {
  return e - 2 * (8 * S - 2) + 8 * (S - 1);
}

}  // namespace gpbo
