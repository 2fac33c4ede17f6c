// r2, the variance ratio of a truncated unit normal, as a device function: gpje_jes_argbest (jes.hip) and gpmf_mes_argbest (mfmes.hip)
// evaluate the same text, so the two give the same bits.  include/gpje.h has the ranges.  Both callers compile with -ffp-contract=off.
#pragma once

#include "gpbo_internal.h"
#include "acq_formulas.h"

#include <cmath>

namespace gpbo {

// r2(b) = 1 - b h - h^2, h = phi(b) / Phi(b): the variance of a unit normal truncated to (-inf, b].  include/gpje.h has the ranges.
__device__ __forceinline__ double jes_r2_dev(const double b) {
  if (b != b) return b;
  double out;
  if (b >= -1.0) {
    if (b == INFINITY) return 1.0;      // b h is inf * 0
    const double h = norm_pdf_dev(b) / ndtr_dev(b);
    out = (1.0 - b * h) - h * h;
  } else if (b > -2.0) {
    const double r = log_ei_ratio(b, DevErfcx());
    const double m = (1.0 - r) / (-b);
    out = 1.0 - r / (m * m);
  } else {
    const double x = -b;
    const int n = x >= 10.0 ? 16 : (x >= 6.0 ? 32 : (x >= 3.0 ? 64 : 128));
    double c1 = 0.0, c2 = 0.0;
    for (int k = n; k >= 1; --k) {
      c2 = c1;
      c1 = (double)k / (x + c1);
    }
    out = c1 * (c2 - c1);
  }
  return out < 0.0 ? 0.0 : (out > 1.0 ? 1.0 : out);
}

}  // namespace gpbo
