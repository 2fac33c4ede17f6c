// The optimiser of the one-launch searches in device form: polish_opt.h's steps over ONE wave, lane i = variable i.  Shared by
// polish_fused.hip (polish_rows_kernel: the acquisition local search) and path_ascent.hip (path_ascend_kernel: a posterior function
// draw climbed to its maximiser) — the same code, moved here verbatim from polish_fused.hip, so both walks take the same decisions.
#pragma once

#include "gpbo_internal.h"
#include "polish_opt.h"
#include "posterior_rows.h"

namespace gpbo {

static_assert(POLISH_OPT_PAIRS == LBFGS_M, "search_plan.h sizes the optimiser's LDS block for polish_opt.h's correction pairs");

// ---- the optimiser: polish_opt.h's steps over wave 0, lane i = variable i (d <= 64; lanes >= d carry zeros) ---------------------
// Against the host's arithmetic: (a) a sum over the variables is a DPP butterfly inside the rows of 16
// lanes + the rows' totals (the host's left-to-right chain would be 3 d instructions of v_readlane + add); (b) s.y and y.y of a correction pair are kept from the step that
// stored it — the recursion recomputes them only while some variable sits on a bound (the sums then run over the free variables);
// (c) the CODE is kept short: the two loops of the recursion are ONE rolled loop with one reduction in its body, the new direction
// is formed at one place.  (c) is what the time hangs on: with every loop unrolled and the routines inlined at each call site the
// kernel was 65 KB of instructions, more than the instruction cache two CUs share — in-kernel clocks: 8-9 000 cycles per step AND
// the evaluation beside it 14 000 instead of the 8 200 it takes alone (profiles/r06_polish_fused_ab.json, notes).
template <int CTRL>
__device__ __forceinline__ double pr_dpp(double v) {      // v of the lane the DPP pattern CTRL pairs this one with (inside a row of 16)
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror: after the four steps every lane holds its row's total
__device__ __forceinline__ double pr_sum(double v, int d) {      // lanes >= d carry zeros
#pragma clang fp contract(off)
  v += pr_dpp<0xB1>(v);
  v += pr_dpp<0x4E>(v);
  v += pr_dpp<0x141>(v);
  v += pr_dpp<0x140>(v);
  double acc = pr_lane(v, 0);
  if (d > 16) acc += pr_lane(v, 16);
  if (d > 32) acc = (acc + pr_lane(v, 32)) + pr_lane(v, 48);
  return acc;
}
__device__ __forceinline__ double pr_max_abs(double v, int d) {  // max |v_i|, a NaN never wins (polish_opt.h)
  double m = __builtin_fabs(v);
  if (m != m) m = 0.0;
  m = polish_max(m, pr_dpp<0xB1>(m));
  m = polish_max(m, pr_dpp<0x4E>(m));
  m = polish_max(m, pr_dpp<0x141>(m));
  m = polish_max(m, pr_dpp<0x140>(m));
  double acc = pr_lane(m, 0);
  if (d > 16) acc = polish_max(acc, pr_lane(m, 16));
  if (d > 32) acc = polish_max(polish_max(acc, pr_lane(m, 32)), pr_lane(m, 48));
  return acc;
}

struct RowsRun {
  double x, g, xt, dir, lo, hi;        // this lane's variable
  bool freev;
  double f, alpha;
  int hist, head, iter, evals, ls, phase, status;
};
// one answer (ft, this lane's gradient component gt — non-finite components already 0) of the objective: polish_advance
// (opt: the optimiser's LDS block, search_plan.h's polish_opt_doubles)
__device__ __forceinline__ void pr_advance(RowsRun& r, double ft, double gt, int d, int lane, double* opt, int max_iter) {
#pragma clang fp contract(off)
  double* S = opt;
  double* Y = S + LBFGS_M * d;
  double* SY = Y + LBFGS_M * d;
  double* YY = SY + LBFGS_M;
  double* RHO = YY + LBFGS_M;
  double* AV = RHO + LBFGS_M;
  const bool mine = lane < d;
  ++r.evals;
  bool fresh = false;      // a new direction is due
  if (r.phase == 0) {
    r.x = r.xt; r.g = gt; r.f = ft;
    if (!__builtin_isfinite(ft)) { r.phase = 2; r.status = 2; return; }
    r.phase = 1;
    fresh = true;
  } else {
    const double sd = r.xt - r.x;
    const double gs = pr_sum(r.g * sd, d), moved = pr_max_abs(sd, d);
    const bool ok = __builtin_isfinite(ft) && ft <= r.f + 1e-4 * gs;
    if (!ok) {
      const bool flat = __builtin_isfinite(ft) && r.ls >= 2 &&
                        __builtin_fabs(ft - r.f) <= POLISH_FTOL * polish_max(polish_max(__builtin_fabs(ft), __builtin_fabs(r.f)), 1.0);
      if (moved == 0.0 || flat) { r.phase = 2; r.status = 1; return; }
      if (++r.ls >= POLISH_MAXLS) { r.phase = 2; r.status = 3; return; }
      double shrink = 0.1;
      if (__builtin_isfinite(ft)) {
        const double curv = ft - r.f - gs;
        shrink = curv > 0.0 ? polish_min(polish_max(-gs / (2.0 * curv), 0.1), 0.5) : 0.5;
      }
      r.alpha *= shrink;
    } else {
      // accepted: the pair (s, y) joins the ring when it is usable
      const double s = sd, y = gt - r.g;
      const double sy = pr_sum(s * y, d), yy = pr_sum(y * y, d);
      if (sy > 2.2e-16 * yy && yy > 0.0) {
        if (mine) {
          S[r.head * d + lane] = s;
          Y[r.head * d + lane] = y;
        }
        SY[r.head] = sy;
        YY[r.head] = yy;
        r.head = (r.head + 1) % LBFGS_M;
        r.hist = (r.hist + 1 < LBFGS_M) ? r.hist + 1 : LBFGS_M;
      }
      const double f_old = r.f;
      r.x = r.xt; r.g = gt; r.f = ft;
      ++r.iter;
      if ((f_old - ft) <= POLISH_FTOL * polish_max(polish_max(__builtin_fabs(f_old), __builtin_fabs(ft)), 1.0)) {
        // (the projected-gradient test comes first in polish_advance: status 0 wins where both hold)
        r.phase = 2;
        r.status = (pr_max_abs(polish_min(polish_max(r.x - r.g, r.lo), r.hi) - r.x, d) <= POLISH_PGTOL) ? 0 : 1;
        return;
      }
      fresh = true;
    }
  }
  if (fresh) {
    if (pr_max_abs(polish_min(polish_max(r.x - r.g, r.lo), r.hi) - r.x, d) <= POLISH_PGTOL) { r.phase = 2; r.status = 0; return; }
    if (r.iter >= max_iter && r.iter > 0) { r.phase = 2; r.status = 2; return; }
    // ---- the new direction: two-loop recursion over the free variables (polish_new_direction)
    r.freev = mine && !((r.x <= r.lo && r.g > 0.0) || (r.x >= r.hi && r.g < 0.0));
    const bool allfree = __ballot(r.freev) == __ballot(mine);
    int usable = 0, used = 0;          // bit t: the t-th newest pair takes part
    double gamma = 1.0;
    for (int t = 0; t < r.hist; ++t) {
      const int k = (r.head - 1 - t + 2 * LBFGS_M) % LBFGS_M;
      double sy = SY[k], yy = YY[k];
      if (!allfree) {
        const double s = mine ? S[k * d + lane] : 0.0, y = mine ? Y[k * d + lane] : 0.0;
        sy = pr_sum(r.freev ? s * y : 0.0, d);
        yy = pr_sum(r.freev ? y * y : 0.0, d);
      }
      if ((sy > 2.2e-16 * yy) && (yy > 0.0)) {
        usable |= 1 << t;
        RHO[k] = 1.0 / sy;
        if (used == 0) gamma = sy / yy;
        ++used;
      }
    }
    double q = r.freev ? r.g : 0.0;
    // j < hist: the t = j-th newest pair, q -= a_t y_t; then q *= gamma; j >= hist: back from the oldest, q += (a_t - b_t) s_t
    for (int j = 0; j < 2 * r.hist; ++j) {
      const bool first = j < r.hist;
      const int t = first ? j : 2 * r.hist - 1 - j;
      if (j == r.hist) q *= gamma;
      if (!((usable >> t) & 1)) continue;
      const int k = (r.head - 1 - t + 2 * LBFGS_M) % LBFGS_M;
      const double s = mine ? S[k * d + lane] : 0.0, y = mine ? Y[k * d + lane] : 0.0;
      const double dot = pr_sum(r.freev ? (first ? s : y) * q : 0.0, d);
      const double c = RHO[k] * dot;
      if (first) {
        AV[k] = c;
        if (r.freev) q -= c * y;
      } else {
        if (r.freev) q += (AV[k] - c) * s;
      }
    }
    if (r.hist == 0) q *= gamma;
    r.dir = r.freev ? -q : 0.0;
    const double gd = pr_sum(r.dir * r.g, d), gn = pr_sum(r.freev ? r.g * r.g : 0.0, d);
    if (!(gd < 0.0) || !__builtin_isfinite(gd)) {     // not a descent direction: steepest descent over the free variables, history dropped
      r.hist = 0;
      used = 0;
      r.dir = r.freev ? -r.g : 0.0;
    }
    r.alpha = (used == 0) ? polish_min(1.0, 1.0 / __builtin_sqrt(polish_max(gn, 1e-300))) : 1.0;
    r.ls = 0;
  }
  r.xt = polish_min(polish_max(r.x + r.alpha * r.dir, r.lo), r.hi);      // the trial point (polish_trial_point)
}

}  // namespace gpbo
