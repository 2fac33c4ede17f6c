// The host-side arithmetic of a scaled model  K = c * k + (w + a) * I  (ConstantKernel * k + WhiteKernel in scikit-learn's terms;
// c = constant_value, w = noise_level, a = the estimator's alpha, k = a unit-amplitude kernel of gpbo.h).  Host-only and free of
// HIP: tests/test_scaled_kernel_host.py compiles it with the system C++ compiler and checks it against scikit-learn.
//
// The reduction.  K = c * K', K' = k + eta * I with eta = (w + a) / c, so the device fits the UNIT model at noise eta and keeps
// L', W' = L'^-1 and alpha' = K'^-1 y; no factorisation kernel, k* generator or GEMM knows about c or w:
//   L_ = sqrt(c) L',  alpha_ = alpha' / c,  mu = y_std (k* . alpha') + y_mean  (unchanged),
//   sigma = y_std sqrt(max(c (1 - q) + w, 0)) with q = |W' k*|^2,  cov = y_std^2 (c (k(X, X) - V^T V) + w I) with V = W' K*^T,
//   LML(c, l, w) = U - (N / 2) log c, U = the unit model's LML of the targets y / sqrt(c) at noise eta.
// With alpha'' = K'^-1 (y / sqrt(c)) and g_eta = 0.5 (|alpha''|^2 - tr K'^-1) — U's gradient component for dK'/dtheta = I, one
// more word of the device's gradient reduction (lml_bodies.h) —
//   d LML / d log l = U's own gradient,
//   d LML / d log w = (w / c) g_eta,
//   d LML / d log c = 0.5 ((y / sqrt(c))^T alpha'' - N) - eta g_eta      ((y / sqrt(c))^T alpha'' is U's first output word).
#pragma once

#include <cmath>
#include <cstdint>

namespace gpbo {

// amplitude > 0, white >= 0, both finite
inline bool scaled_args_ok(double amplitude, double white) {
  return std::isfinite(amplitude) && std::isfinite(white) && amplitude > 0.0 && white >= 0.0;
}

// the noise of the unit model: (w + a) / c.  At c = 1, w = 0 it is a itself, bit for bit.
inline double scaled_eta(double amplitude, double white, double alpha) { return (white + alpha) / amplitude; }

// the factor on the targets of an LML evaluation: y / sqrt(c) = y * scaled_target_scale(c).  Exactly 1 at c = 1.
inline double scaled_target_scale(double amplitude) { return 1.0 / std::sqrt(amplitude); }

// LML(c, l, w) from U
inline double scaled_lml(double unit_lml, int64_t N, double amplitude) {
  return unit_lml - 0.5 * (double)N * std::log(amplitude);      // log(1) is an exact 0
}

// grad[0 .. n_ls + 1] = d LML / d [log c, log l ..., log w] from the unit evaluation's words: yta = (y / sqrt(c))^T alpha'',
// g_ls[n_ls] = U's gradient, g_eta as above.
inline void scaled_lml_gradient(double amplitude, double white, double alpha, int64_t N, double yta, const double* g_ls, int n_ls,
                                double g_eta, double* grad) {
  grad[0] = 0.5 * (yta - (double)N) - scaled_eta(amplitude, white, alpha) * g_eta;
  for (int t = 0; t < n_ls; ++t) grad[1 + t] = g_ls[t];
  grad[1 + n_ls] = (white / amplitude) * g_eta;
}

// scikit-learn's fitted quantities from the unit model's: K = c K', L_ = sqrt(c) L', alpha_ = alpha' / c
// (entry by entry; at c = 1 each returns its argument's bits)
inline double scaled_K_entry(double amplitude, double k_unit) { return amplitude * k_unit; }
inline double scaled_L_entry(double amplitude, double l_unit) { return std::sqrt(amplitude) * l_unit; }
inline double scaled_alpha_entry(double amplitude, double alpha_unit) { return alpha_unit / amplitude; }

}  // namespace gpbo
