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

}  // namespace gpbo
