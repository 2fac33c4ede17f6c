// norm.cdf / norm.pdf as the acquisition kernels evaluate them (scipy.special.ndtr, Cephes: 0.5 + 0.5 erf(x / sqrt2) for
// |x / sqrt2| < sqrt(.5), else 0.5 erfc(|x| / sqrt2) reflected; exp(-x^2 / 2) / sqrt(2 pi), scipy _continuous_distns.py:360-369).
// Shared by acq_kernels.hip and evolve.hip; both compile with -ffp-contract=off, so the two give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace gpbo {

__device__ __forceinline__ double ndtr_dev(double a) {
  if (a != a) return a;
  const double x = a * 0.70710678118654752440;  // a * sqrt(1/2)
  const double z = fabs(x);
  double y;
  if (z < 0.70710678118654752440) {
    y = 0.5 + 0.5 * erf(x);
  } else {
    y = 0.5 * erfc(z);
    if (x > 0) y = 1.0 - y;
  }
  return y;
}

__device__ __forceinline__ double norm_pdf_dev(double x) {
  return exp(-(x * x) / 2.0) / 2.50662827463100050242;  // sqrt(2*pi)
}

// ---- log expected improvement (GPBO_ACQ_LOG_EI; include/gpbo.h has the definition and the conventions) ----------------------------
// logEI = log(sd) + log h(z), h(z) = phi(z) + z Phi(z).  Below z = -1 the sum cancels (and underflows at z ~ -38.5), so h is
// written as phi(z) r(z), r = 1 + z Phi(z) / phi(z):
//   -28 < z <= -1   r = 1 - sqrt(pi) t erfcx(t), t = -z / sqrt2      (the cancellation costs z^2 eps: the (1 + z^2) every caller's
//                                                                     error model carries for the division that made z)
//   z <= -28        r = w (1 - 3 w + 15 w^2 - ...), w = 1 / z^2: ten terms of the asymptotic series of Mills' ratio, the first one
//                   left out below 2e-19 there.  (w = 0 for |z| > 1e154: log r = -inf, the value's lower end.)
// `erfcx_of` is the caller's scaled complementary error function: the device library's here and in polish_fused.hip, polish.hip's
// erfcx_host (exp(t^2) erfc(t) with the rounding of t^2 put back; t < 19.8: erfc is far from its underflow) on the host side.
constexpr double LOG_EI_SERIES_BELOW = -28.0;
constexpr double LOG_EI_HALF_LOG_2PI = 0.91893853320467274178;  // log(2 pi) / 2

template <class Erfcx>
__host__ __device__ __forceinline__ double log_ei_ratio(double z, Erfcx&& erfcx_of) {      // r(z), z <= -1
#pragma clang fp contract(off)
  if (z > LOG_EI_SERIES_BELOW) {
    const double t = -z * 0.70710678118654752440;
    return 1.0 - 1.77245385090551602730 * t * erfcx_of(t);      // sqrt(pi)
  }
  const double w = 1.0 / (z * z);
  double s = -654729075.0;      // (2k + 1)!!, k = 9 ... 0, alternating
  s = s * w + 34459425.0;
  s = s * w - 2027025.0;
  s = s * w + 135135.0;
  s = s * w - 10395.0;
  s = s * w + 945.0;
  s = s * w - 105.0;
  s = s * w + 15.0;
  s = s * w - 3.0;
  s = s * w + 1.0;
  return w * s;
}

struct DevErfcx {
  __device__ __forceinline__ double operator()(double t) const { return erfcx(t); }
};

// log h(z); NaN for a NaN z
__device__ __forceinline__ double log_h_dev(double z) {
  if (z > -1.0) return log(norm_pdf_dev(z) + z * ndtr_dev(z));
  return -(z * z) / 2.0 - LOG_EI_HALF_LOG_2PI + log(log_ei_ratio(z, DevErfcx()));
}

// logEI from aa = mu - y_max - xi and sd.  A clipped variance (sd == 0) leaves the improvement itself: log(aa), -inf for aa <= 0.
__device__ __forceinline__ double log_ei_dev(double aa, double sd) {
  if (sd == 0.0) return (aa != aa) ? aa : (aa > 0.0 ? log(aa) : -INFINITY);
  return log(sd) + log_h_dev(aa / sd);
}

// ---- log feasibility (GPBO_ACQ_LOG_CEI / GPBO_ACQ_LOG_FEAS; include/gpbo.h has the definition and the conventions) ---------------
// log p_j = log(Phi(b) - Phi(a)), a = (lb - cm) / cs, b = (ub - cm) / cs, without the subtraction of two numbers near 0 or near 1
// that makes the product form's p_j exactly 0 a few sigma outside the band.  `ndtr_of` / `erfcx_of` are the caller's Phi and scaled
// complementary error function: ndtr_dev and the device library's erfcx here, polish.hip's norm_cdf and erfcx_tail_host on the host
// side of gpbo_polish_seeds.
constexpr double LOG_FEAS_LOG_2 = 0.69314718055994530942;
constexpr double LOG_FEAS_RSQRT2 = 0.70710678118654752440;

// log Phi(x): log(ndtr(x)) above -1; below it Phi = erfc(t) / 2 = exp(-t^2) erfcx(t) / 2 with t = -x / sqrt2, which does not underflow
template <class Ndtr, class Erfcx>
__host__ __device__ __forceinline__ double log_ndtr_of(double x, Ndtr&& ndtr_of, Erfcx&& erfcx_of) {
#pragma clang fp contract(off)
  if (x > -1.0) return log(ndtr_of(x));
  if (!(x <= -1.0)) return x;      // NaN
  return -(x * x) / 2.0 + log(erfcx_of(-x * LOG_FEAS_RSQRT2)) - LOG_FEAS_LOG_2;
}

// log(Phi(b) - Phi(a)) of a finite two-sided band in standardised units.  a == b: -inf; a > b or a NaN: NaN.  An interval in the
// upper tail is reflected into the lower one first.  Then
//   a <= -1, b <= 0   log Phi(b) + log(-expm1(log Phi(a) - log Phi(b)))      both in one tail, Phi(a) small
//   a > -1,  b <= 0   log((erf(b / sqrt2) - erf(a / sqrt2)) / 2)             both within one sigma below the centre: the difference of
//                     the two log Phi would lose |log Phi| Phi / (phi |a|) against the band's own condition number there (3 at -0.3,
//                     without bound towards 0), the difference of the two erf — each of size ~ 0.8 |x| — loses nothing
//   a < 0 < b         log((erf(b / sqrt2) + erf(-a / sqrt2)) / 2)            straddling: two positive terms
template <class Ndtr, class Erfcx>
__host__ __device__ __forceinline__ double log_band_of(double a, double b, Ndtr&& ndtr_of, Erfcx&& erfcx_of) {
#pragma clang fp contract(off)
  if (a != a || b != b || a > b) return __builtin_nan("");
  if (a == b) return -__builtin_inf();
  if (a >= 0.0) { const double t = a; a = -b; b = -t; }
  if (b <= 0.0) {
    if (a > -1.0) return log(0.5 * (erf(b * LOG_FEAS_RSQRT2) - erf(a * LOG_FEAS_RSQRT2)));
    const double lpb = log_ndtr_of(b, ndtr_of, erfcx_of), lpa = log_ndtr_of(a, ndtr_of, erfcx_of);
    return lpb + log(-expm1(lpa - lpb));
  }
  return log(0.5 * (erf(b * LOG_FEAS_RSQRT2) + erf(-a * LOG_FEAS_RSQRT2)));
}

// log p_j of one constraint from its bounds and posterior (cm, cs): 0 for two infinite bounds (the posterior is not looked at, as
// the product form's p_j = 1 - 0), NaN unless cs > 0 (cdf_loc_scale's rule); `a_out` / `b_out` get the standardised bounds (-inf /
// +inf for an infinite one, without a division) for the gradient's coefficients
template <class Ndtr, class Erfcx>
__host__ __device__ __forceinline__ double log_interval_of(double lb, double ub, double cm, double cs, Ndtr&& ndtr_of, Erfcx&& erfcx_of,
                                                           double& a_out, double& b_out) {
#pragma clang fp contract(off)
  const bool has_lb = lb != -__builtin_inf(), has_ub = ub != __builtin_inf();
  a_out = -__builtin_inf(); b_out = __builtin_inf();
  if (!has_lb && !has_ub) return 0.0;
  if (!(cs > 0.0)) return __builtin_nan("");
  if (has_lb) a_out = (lb - cm) / cs;
  if (has_ub) b_out = (ub - cm) / cs;
  if (!has_lb) return log_ndtr_of(b_out, ndtr_of, erfcx_of);
  if (!has_ub) return log_ndtr_of(-a_out, ndtr_of, erfcx_of);
  return log_band_of(a_out, b_out, ndtr_of, erfcx_of);
}

struct DevNdtr {
  __device__ __forceinline__ double operator()(double x) const { return ndtr_dev(x); }
};

__device__ __forceinline__ double log_ndtr_dev(double x) { return log_ndtr_of(x, DevNdtr(), DevErfcx()); }

__device__ __forceinline__ double log_interval_dev(double lb, double ub, double cm, double cs) {
  double a, b;
  return log_interval_of(lb, ub, cm, cs, DevNdtr(), DevErfcx(), a, b);
}

}  // namespace gpbo
