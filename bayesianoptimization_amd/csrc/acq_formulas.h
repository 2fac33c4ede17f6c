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

}  // namespace gpbo
