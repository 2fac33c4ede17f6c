// Max-value entropy search (Wang & Jegelka 2017) over the resident candidates (gfx950): gpbo_mes_argbest's values.
//   gamma_s(x) = (y*_s - mu(x)) / sd(x)
//   a(x)       = 1/S sum_s h(gamma_s(x)),      h(g) = g phi(g) / (2 Phi(g)) - log Phi(g)
//   ys[i]      = -a(x_i)                       the key the selection launches of acq_kernels.hip minimise
// Compiled with -ffp-contract=off, as acq_kernels.hip: acq_formulas.h's pieces give the bits they give there.
//
// h over its three ranges (include/gpbo.h has the conventions):
//   -1 < g <= 0   the formula as written, ndtr_dev / norm_pdf_dev.
//   g > 0         through the complement q = Phi(-g) = erfc(g / sqrt2) / 2:  h = g phi / (2 (1 - q)) - log1p(-q).  log(Phi) of a Phi
//                 rounded next to 1 is 0.2 % off at g = 8 and 0.9 % at g = 15.  From g = 40 on phi and q are 0 and so is h (g is cut there: inf * 0).
//   g <= -1       the two halves each grow like g^2 / 2 and cancel.  r = log_ei_ratio(g) = 1 + g Phi / phi (erfcx down to -28, the
//                 series below), the lower-tail Mills ratio m = (1 - r) / (-g) = Phi / phi, and
//                    h = g r / (2 m) + log(2 pi) / 2 - log m
//                 which grows like log|g|.  Below -1e150 (1 / g^2 leaves the normal range at 1e154) h is its own limit
//                 -1/2 + log(2 pi) / 2 + log(-g), exact to ~1 / g^2.
//
// Lanes DIVERGE over the three ranges; they do not evaluate two forms and select.  A y* is a sampled maximum of the posterior, so
// for nearly every candidate gamma > 0 and a wave runs the complement branch alone; evaluating the tail form beside it would add
// an erfcx and a second log to every lane of every wave to save the waves that straddle a boundary (and erf / erfc / erfcx of the
// device library branch on their argument inside anyway).  A straddling wave pays the sum of the branches it holds.
//
// Thread = candidate, grid-stride.  The sum over s runs s = 0 .. S - 1 in that order, then ONE division by S: a candidate's bits do
// not depend on M, on the grid or on the other candidates.  y* rides in the kernarg struct: every lane reads the same word, a
// scalar load per sample.  1 / sd once per candidate.  fp64 whatever the slot's precision.
#include "gpbo_internal.h"
#include "acq_formulas.h"

#include <cmath>

namespace gpbo {

struct MesDev {
  const double* mu;
  const double* sd;
  int n_samples;
  double y_star[GPBO_MAX_MES_SAMPLES];
};

constexpr double MES_ZERO_FROM = 40.0;        // phi(40) = exp(-800) / sqrt(2 pi) = 0 and Phi(-40) = 0 in fp64: h = 0
constexpr double MES_LIMIT_BELOW = -1e150;

// h(g) >= 0, strictly decreasing; NaN for a NaN g, +inf at -inf, 0 from MES_ZERO_FROM on
__device__ __forceinline__ double mes_h_dev(double g) {
  if (g != g) return g;
  if (g > 0.0) {
    if (g > MES_ZERO_FROM) g = MES_ZERO_FROM;
    const double q = 0.5 * erfc(g * 0.70710678118654752440);
    return g * norm_pdf_dev(g) / (2.0 * (1.0 - q)) - log1p(-q);
  }
  if (g > -1.0) {
    const double cdf = ndtr_dev(g);
    return g * norm_pdf_dev(g) / (2.0 * cdf) - log(cdf);
  }
  if (g < MES_LIMIT_BELOW) return -0.5 + LOG_EI_HALF_LOG_2PI + log(-g);
  const double r = log_ei_ratio(g, DevErfcx());
  const double m = (1.0 - r) / (-g);
  return g * r / (2.0 * m) + LOG_EI_HALF_LOG_2PI - log(m);
}

// -a(x_i).  A clipped variance (sd == 0) carries no information: 0, unless mu is NaN; a NaN mu or sd gives NaN.
__device__ __forceinline__ double mes_value(const MesDev& a, const int64_t i) {
  const double mean = a.mu[i], sd = a.sd[i];
  if (mean != mean) return mean;
  if (sd != sd) return sd;
  if (sd == 0.0) return -0.0;
  const double inv = 1.0 / sd;
  double acc = 0.0;
  for (int s = 0; s < a.n_samples; ++s) acc = acc + mes_h_dev((a.y_star[s] - mean) * inv);
  return -(acc / (double)a.n_samples);
}

__global__ __launch_bounds__(256) void mes_kernel(MesDev a, int64_t M, double* __restrict__ ys) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += stride) ys[i] = mes_value(a, i);
}

constexpr int64_t MES_MAX_BLOCKS = 8192;      // 32 blocks of 4 waves for each of 256 compute units; the stride loop takes the rest

int launch_mes_values(gpbo_ctx* ctx, const Model& m, int64_t M, int n_samples, const double* y_star) {
  int rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  MesDev a{};
  a.mu = m.mu; a.sd = m.sd; a.n_samples = n_samples;
  for (int s = 0; s < n_samples; ++s) a.y_star[s] = y_star[s];
  const int64_t blocks = (M + 255) / 256;
  mes_kernel<<<dim3((unsigned)(blocks < MES_MAX_BLOCKS ? blocks : MES_MAX_BLOCKS)), dim3(256), 0, ctx->stream>>>(a, M, ctx->ys);
  GPBO_HIP(ctx, hipGetLastError());
  return GPBO_OK;
}

}  // namespace gpbo
