// gpbo_evolve_mixed: the differential evolution of a mixed-space smart stage as ONE workgroup on the device.
//
// What it replaces: the DifferentialEvolutionSolver(func=acq, bounds, init=population, polish=False, rng=random_state).solve() of
// bayes_opt/acquisition.py:375-396 (fused_acquisition.py, _evolve_mixed), in which SciPy calls the objective one point at a time —
// on the accelerated path one Python -> ctypes -> device round trip per trial, about 1 000 of them per suggest().  Here the walk and
// its evaluations stay on the device: SciPy 1.15's solver in the configuration the reference uses (best1bin, mutation (0.5, 1)
// dithered, recombination 0.7, updating 'immediate', tol 0.01, atol 0, no integrality / constraints / callback / maxfun), draw for
// draw on the caller's legacy MT19937 RandomState (tests/de_walk.py states it op by op; tests/test_evolve_host.py holds that
// statement to SciPy bit for bit):
//   init       population = clip((init - arg1) * recip + 0.5, 0, 1), recip = 1 / |hi - lo| with non-finite entries 0; every member
//              evaluated in order, the lowest energy promoted to row 0 (np.argmin: the first NaN wins)
//   generation (all energies infinite: the whole population evaluated again first) scale = uniform(0.5, 1); per candidate c:
//              fill = randint(0, D) (no word when D = 1) | shuffle of the persistent index array (S - 1 masked-rejection draws) |
//              r0, r1 = the first two of its first 6 entries that are not c | bprime = pop[0] + scale (pop[r0] - pop[r1]) |
//              crossover = uniform(size=D) < 0.7, forced at fill | out-of-range coordinates redrawn by uniform(size=oob) | the trial
//              replaces c when energy <= E[c], and is promoted when also energy <= E[0]
//   stop       after a generation: no energy infinite and std(E) <= 0 + 0.01 |mean(E)| (NumPy's pairwise float64 sums), else on at
//              most maxiter generations (success = false)
// The objective at a trial x: TargetSpace.kernel_transform per column group (identity / rint / one-hot at the first argmax, row-local for
// one row), the posterior of slot 0 with thread = training point (posterior_rows.h, the evaluation of polish_fused.hip: W in LDS for
// NP <= 128 when it fits, its transposed copy streamed from memory up to 512: search_plan.h's plan_evolve), then -base_acq(mu, sd) with the acquisition kernels'
// formulas (acq_formulas.h).  Values agree with the host's objective to rounding; the walk is the host solver's as long as no
// comparison of two energies falls within that rounding.
// Wave 0 runs the solver (every lane the same uniform steps; lane t holds coordinate t); the state — population, energies, index
// array, MT19937 words and position, scale, counters — lives in device memory between launches and in LDS during one.  A launch
// stops at the first candidate boundary after `budget` evaluations and the host launches again until the run has ended, so that no
// launch holds the GPU for more than a few milliseconds.  Compiled with -ffp-contract=off: scaling and mutation round as NumPy does.
#include <algorithm>
#include <cmath>
#include <vector>

#include "acq_formulas.h"
#include "gpbo_internal.h"
#include "posterior_rows.h"

namespace gpbo {

namespace {

enum EvPhase { PH_PASS = 0, PH_GEN = 1, PH_SCALE = 2, PH_CAND = 3, PH_DONE = 4 };

struct EvolveArgs {
  // objective: slot 0's posterior (analytic = 0) or the debug walk's analytic sum (analytic = 1)
  const double *W, *Wt, *Xs, *alpha, *ls;
  int NP, N, DP;
  double y_mean, y_std;
  double amplitude, white;             // of slot 0's model: normalised variance = amplitude * (1 - |W k*|^2) + white
  int acq;
  double acq_param, y_max;
  int analytic;
  const double *aw, *aa;               // (D,) weights and targets of the analytic objective
  double nan_below, inf_above;         // analytic: NaN where x_0 < nan_below, +inf where x_0 > inf_above
  // space: per column its kind (0 float, 1 int, 2 categorical) and its group's first column / width; the scaling of SciPy's solver
  int D, S, maxiter, budget;
  const int *ckind, *cg0, *cgn;
  const double *arg1, *arg2;
  // state
  double* pop;                         // (S, D) in [0, 1]
  double* energies;                    // (S,)
  int* perm;                           // (S,) _random_population_index
  unsigned* mt;                        // (624,) the untempered MT19937 key
  int* ist;                            // EvInt words
  double* scale;                       // (1,)
  // eval-only (debug): f at n points (n, D) in parameter space
  int eval_n;
  const double* eval_x;
  double* eval_out;
  int pop_lds;                         // the population fits the LDS
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- MT19937 on wave 0 (every lane the same value) ------------------------------------------------------------------------------
struct Mt {
  unsigned* key;   // LDS
  int pos;
  // the regeneration: 624 words in chunks of 64 lanes, in order.  Word i reads words i + 1 (old: a later chunk or a later lane of
  // this one, whose store follows this load) and (i + 397) mod 624 (old for i < 227; for i >= 227 the NEW word i - 227, written at
  // least two chunks earlier) — the serial loop's values.
  __device__ void twist(int lane) {
    for (int base = 0; base < 624; base += 64) {
      const int i = base + lane;
      unsigned v = 0;
      if (i < 624) {
        const unsigned cur = key[i], nxt = key[(i + 1) % 624], far = key[(i + 397) % 624];
        const unsigned y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
        v = far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      wave_sync();
      if (i < 624) key[i] = v;
      wave_sync();
    }
  }
  __device__ unsigned next(int lane) {
    if (pos >= 624) {
      twist(lane);
      pos = 0;
    }
    unsigned y = key[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
  __device__ double dbl(int lane) {
    const unsigned a = next(lane) >> 5, b = next(lane) >> 6;
    return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
  }
  __device__ int interval(unsigned mx, int lane) {      // random_interval: masked rejection
    if (mx == 0) return 0;
    unsigned mask = mx;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    unsigned v;
    while ((v = (next(lane) & mask)) > mx) {
    }
    return (int)v;
  }
};

// np.argmin over E (first NaN, else the first smallest), wave 0
__device__ int ev_argmin(const double* E, int S, int lane) {
  int best = -1, nan_at = -1;
  double bv = 0.0;
  for (int i = lane; i < S; i += 64) {
    const double v = E[i];
    if (v != v) { if (nan_at < 0) nan_at = i; continue; }
    if (best < 0 || v < bv) { best = i; bv = v; }
  }
  int gbest = -1, gnan = -1;
  double gv = 0.0;
  for (int l = 0; l < 64; ++l) {
    const int bn = __builtin_amdgcn_readlane(nan_at, l);
    const int bi = __builtin_amdgcn_readlane(best, l);
    const double v = pr_lane(bv, l);
    if (bn >= 0 && (gnan < 0 || bn < gnan)) gnan = bn;
    if (bi >= 0 && (gbest < 0 || v < gv || (v == gv && bi < gbest))) { gbest = bi; gv = v; }
  }
  return gnan >= 0 ? gnan : (gbest >= 0 ? gbest : 0);
}

// NumPy's pairwise float64 sum of f(E[i]) (8 accumulators up to 128 values, halves above), uniform over wave 0.  The recursion runs
// on an explicit stack in LDS (EV_STACK frames: lo, n, state; partial sums), post-order: left half, right half, left + right.
template <class F>
__device__ double ev_pairwise(const double* E, int n0, int* frames, double* acc, F f) {
#pragma clang fp contract(off)
  int sp = 0, top = 0;
  frames[0] = 0; frames[1] = n0; frames[2] = 0;
  sp = 1;
  while (sp > 0) {
    int* fr = frames + 3 * (sp - 1);
    const int lo = fr[0], n = fr[1], state = fr[2];
    if (n <= 128) {
      double res;
      if (n < 8) {
        res = 0.0;
        for (int i = 0; i < n; ++i) res += f(E[lo + i]);
      } else {
        double r0 = f(E[lo]), r1 = f(E[lo + 1]), r2 = f(E[lo + 2]), r3 = f(E[lo + 3]), r4 = f(E[lo + 4]), r5 = f(E[lo + 5]),
               r6 = f(E[lo + 6]), r7 = f(E[lo + 7]);
        int i = 8;
        for (; i < n - (n % 8); i += 8) {
          const double* e = E + lo + i;
          r0 += f(e[0]); r1 += f(e[1]); r2 += f(e[2]); r3 += f(e[3]); r4 += f(e[4]); r5 += f(e[5]); r6 += f(e[6]); r7 += f(e[7]);
        }
        res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < n; ++i) res += f(E[lo + i]);
      }
      wave_sync();
      acc[top++] = res;
      --sp;
      wave_sync();
      continue;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    wave_sync();
    if (state == 0) {
      fr[2] = 1;
      int* nf = frames + 3 * sp++;
      nf[0] = lo; nf[1] = n2; nf[2] = 0;
    } else if (state == 1) {
      fr[2] = 2;
      int* nf = frames + 3 * sp++;
      nf[0] = lo + n2; nf[1] = n - n2; nf[2] = 0;
    } else {
      const double right = acc[top - 1], left = acc[top - 2];
      wave_sync();
      top -= 2;
      acc[top++] = left + right;
      --sp;
    }
    wave_sync();
  }
  return acc[0];
}

__device__ bool ev_converged(const double* E, int S, int* frames, double* acc) {
#pragma clang fp contract(off)
  for (int i = 0; i < S; ++i)
    if (__builtin_isinf(E[i])) return false;
  const double mean = ev_pairwise(E, S, frames, acc, [](double v) { return v; }) / (double)S;
  const double var = ev_pairwise(E, S, frames, acc, [mean](double v) { const double dv = v - mean; return dv * dv; }) / (double)S;
  return sqrt(var) <= 0.0 + 0.01 * fabs(mean);
}

// wave 0: kernel_transform of the point px (LDS, D columns) over the length scales into xs (DP columns, zero padded)
__device__ void ev_transform(const EvolveArgs& a, const double* px, const double* ls_s, double* xs, int lane) {
  if (lane < a.DP) {
    double v = 0.0;
    if (lane < a.D) {
      const int kind = a.ckind[lane];
      v = px[lane];
      if (kind == 1) {
        v = rint(v);
      } else if (kind == 2) {
        const int g0 = a.cg0[lane], gn = a.cgn[lane];
        int best = 0;
        double bv = px[g0];
        if (bv == bv)
          for (int c = 1; c < gn; ++c) {
            const double w = px[g0 + c];
            if (w != w) { best = c; break; }
            if (w > bv) { bv = w; best = c; }
          }
        v = (lane - g0 == best) ? 1.0 : 0.0;
      }
      v = v / ls_s[lane];
    }
    xs[lane] = v;
  }
}

// wave 0: the analytic objective of the debug walk, sum_t w_t (g_t - a_t)^2 left to right
__device__ double ev_analytic(const EvolveArgs& a, const double* px) {
#pragma clang fp contract(off)
  if (px[0] < a.nan_below) return __builtin_nan("");
  if (px[0] > a.inf_above) return __builtin_inf();
  double s = 0.0;
  for (int t = 0; t < a.D; ++t) {
    const double g = a.ckind[t] == 1 ? rint(px[t]) : px[t];
    const double dl = g - a.aa[t];
    s = s + a.aw[t] * (dl * dl);
  }
  return s;
}

template <int KERNEL, bool WLDS>
__global__ __launch_bounds__(SEARCH_MAX_NP) void evolve_kernel(const EvolveArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double ev_smem[];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int NP = a.analytic ? 0 : a.NP, N = a.N, D = a.D, S = a.S, DP = a.DP;
  const int WLD = NP + 1;
  const EvolveLds L = evolve_lds(NP, S, D, WLDS, a.pop_lds != 0);
  double *Wl = ev_smem + L.W, *xs = ev_smem + L.xs, *ls_s = ev_smem + L.ls, *px = ev_smem + L.px, *ks = ev_smem + L.ks,
         *vs = ev_smem + L.vs, *pp = ev_smem + L.pp, *E = ev_smem + L.E, *misc = ev_smem + L.misc, *stk_acc = ev_smem + L.acc,
         *popl = ev_smem + L.pop;
  int* const words = (int*)ev_smem;
  unsigned* key = (unsigned*)(words + L.key);
  int *perm = words + L.perm, *frames = words + L.frames;
  double* pop = a.pop_lds ? popl : a.pop;

  if (!a.analytic) {
    if (WLDS) pr_load_w(Wl, a.W, NP, tid);
    if (tid < 64) ls_s[tid] = (tid < D) ? a.ls[tid] : 1.0;
  }
  const int nthr = (int)blockDim.x;
  for (int i = tid; i < S; i += nthr) { E[i] = a.energies[i]; perm[i] = a.perm[i]; }
  for (int i = tid; i < 624; i += nthr) key[i] = a.mt[i];
  if (a.pop_lds)
    for (int i = tid; i < S * D; i += nthr) popl[i] = a.pop[i];
  __syncthreads();

  // ---- solver state (wave 0, uniform)
  Mt mt{key, a.ist[I_POS]};
  int phase = a.ist[I_PHASE], ev = a.ist[I_EV], then = a.ist[I_THEN], c = a.ist[I_C], nit = a.ist[I_NIT], nfev = a.ist[I_NFEV],
      status = a.ist[I_STATUS];
  double scale = a.scale[0];
  double trial = 0.0;      // lane t: coordinate t of the pending trial (unit scale)
  int pending = 0;         // 0 none, 1 a member of a full pass, 2 a candidate, 3 a debug point
  int evals = 0, point = 0;
  const int D1 = D;

  for (;;) {
    if (wave == 0) {
      bool stop = false;
      const double energy = misc[0];
      // (a) the answer to the pending evaluation
      if (pending == 1) {
        if (lane == 0) E[ev] = energy;
        ++nfev;
        ++ev;
        wave_sync();
        if (ev == S) {
          const int l = ev_argmin(E, S, lane);
          if (lane < D1) { const double t0 = pop[lane], tl = pop[(size_t)l * D + lane]; pop[lane] = tl; pop[(size_t)l * D + lane] = t0; }
          if (lane == 0) { const double e0 = E[0]; E[0] = E[l]; E[l] = e0; }
          wave_sync();
          phase = then;
        }
      } else if (pending == 2) {
        ++nfev;
        if (energy <= E[c]) {
          if (lane < D1) pop[(size_t)c * D + lane] = trial;
          wave_sync();
          if (lane == 0) E[c] = energy;
          wave_sync();
          if (energy <= E[0]) {
            const int l = ev_argmin(E, S, lane);
            if (lane < D1) { const double t0 = pop[lane], tl = pop[(size_t)l * D + lane]; pop[lane] = tl; pop[(size_t)l * D + lane] = t0; }
            if (lane == 0) { const double e0 = E[0]; E[0] = E[l]; E[l] = e0; }
            wave_sync();
          }
        }
        ++c;
        if (c == S) {
          if (ev_converged(E, S, frames, stk_acc)) { status = 1; phase = PH_DONE; }
          else phase = PH_GEN;
        }
      } else if (pending == 3) {
        if (lane == 0) a.eval_out[point] = energy;
        ++point;
      }
      pending = 0;
      // (b) on to the next evaluation
      if (a.eval_n > 0) {
        if (point < a.eval_n) {
          if (lane < D) px[lane] = a.eval_x[(size_t)point * D + lane];
          pending = 3;
        } else {
          stop = true;
        }
      } else {
        for (;;) {
          if (phase == PH_DONE || evals >= a.budget) { stop = true; break; }
          if (phase == PH_GEN) {
            if (nit >= a.maxiter) { status = 2; phase = PH_DONE; continue; }
            ++nit;
            bool all_inf = true;
            for (int i = 0; i < S; ++i) all_inf = all_inf && __builtin_isinf(E[i]);
            if (all_inf) { phase = PH_PASS; ev = 0; then = PH_SCALE; }
            else phase = PH_SCALE;
            continue;
          }
          if (phase == PH_SCALE) {
            scale = 0.5 + 0.5 * mt.dbl(lane);
            c = 0;
            phase = PH_CAND;
            continue;
          }
          if (phase == PH_PASS) {
            if (lane < D) {
              const double u = pop[(size_t)ev * D + lane];
              px[lane] = a.arg1[lane] + (u - 0.5) * a.arg2[lane];
            }
            pending = 1;
            break;
          }
          // PH_CAND: the trial of candidate c
          const int fill = mt.interval((unsigned)(D - 1), lane);
          for (int i = S - 1; i > 0; --i) {
            const int j = mt.interval((unsigned)i, lane);
            const int pi = perm[i], pj = perm[j];
            wave_sync();
            if (lane == 0) { perm[i] = pj; perm[j] = pi; }
            wave_sync();
          }
          int r0 = -1, r1 = -1;
          for (int k = 0; k < 6 && k < S; ++k) {
            const int v = perm[k];
            if (v == c) continue;
            if (r0 < 0) r0 = v;
            else if (r1 < 0) r1 = v;
          }
          double bprime = 0.0, cur = 0.0;
          if (lane < D) {
            bprime = pop[lane] + scale * (pop[(size_t)r0 * D + lane] - pop[(size_t)r1 * D + lane]);
            cur = pop[(size_t)c * D + lane];
          }
          bool cross = false;
          for (int t = 0; t < D; ++t) {
            const double u = mt.dbl(lane);
            if (lane == t) cross = u < 0.7;
          }
          if (lane == fill) cross = true;
          trial = cross ? bprime : cur;
          const unsigned long long oob = __ballot(lane < D && (trial > 1.0 || trial < 0.0));
          for (int t = 0; t < D; ++t)
            if ((oob >> t) & 1ull) {
              const double u = mt.dbl(lane);
              if (lane == t) trial = u;
            }
          if (lane < D) px[lane] = a.arg1[lane] + (trial - 0.5) * a.arg2[lane];
          pending = 2;
          break;
        }
      }
      wave_sync();
      if (!stop && a.analytic) {
        const double f = ev_analytic(a, px);
        if (lane == 0) misc[0] = f;
      } else if (!stop) {
        ev_transform(a, px, ls_s, xs, lane);
      }
      if (lane == 0) misc[1] = stop ? 1.0 : 0.0;
      if (!stop) ++evals;
    }
    __syncthreads();
    if (misc[1] != 0.0) break;
    if (a.analytic) continue;
    // ---- the posterior of slot 0 at xs: thread = training point
    {
      double d2;
      const double kv = pr_kstar<KERNEL>(xs, a.Xs + (int64_t)tid * DP, DP, d2);
      ks[tid] = kv;
    }
    __syncthreads();
    double v;
    if (WLDS) {
      v = (tid < N) ? pr_row_lds(Wl + tid * WLD, ks, NP) : 0.0;
    } else {
      pr_rows_mem<4>(a.Wt, ks, NP, N, tid, wave, vs);      // (fewer loads in flight than polish_fused: the solver's registers stay live)
      __syncthreads();
      v = vs[tid];
    }
    pp[2 * tid] = v * v;
    pp[2 * tid + 1] = ks[tid] * a.alpha[tid];
    __syncthreads();
    if (wave == 0) {
      double s2 = 0.0, mm = 0.0;
      for (int k = lane; k < NP; k += 64) {
        s2 += pp[2 * k];
        mm += pp[2 * k + 1];
      }
      for (int off = 32; off >= 1; off >>= 1) {      // a fixed butterfly: every lane ends with the same total
        s2 += __shfl_xor(s2, off);
        mm += __shfl_xor(mm, off);
      }
      s2 = pr_lane(s2, 0);
      mm = pr_lane(mm, 0);
      double var = fma(a.amplitude, 1.0 - s2, a.white);
      if (var < 0.0) var = 0.0;
      const double sd = sqrt(var * (a.y_std * a.y_std));
      const double mu = a.y_std * mm + a.y_mean;
      double base;
      if (a.acq == GPBO_ACQ_UCB) {
        base = mu + a.acq_param * sd;
      } else {
        const double aa = mu - a.y_max - a.acq_param;
        const double z = aa / sd;
        base = (a.acq == GPBO_ACQ_EI) ? aa * ndtr_dev(z) + sd * norm_pdf_dev(z) : ndtr_dev(z);
      }
      if (lane == 0) misc[0] = -1.0 * base;
    }
    __syncthreads();
  }

  if (a.eval_n > 0) return;
  // ---- the state back to memory
  for (int i = tid; i < S; i += nthr) { a.energies[i] = E[i]; a.perm[i] = perm[i]; }
  for (int i = tid; i < 624; i += nthr) a.mt[i] = key[i];
  if (a.pop_lds)
    for (int i = tid; i < S * D; i += nthr) a.pop[i] = popl[i];
  if (tid == 0) {
    a.ist[I_POS] = mt.pos; a.ist[I_PHASE] = phase; a.ist[I_EV] = ev; a.ist[I_THEN] = then; a.ist[I_C] = c; a.ist[I_NIT] = nit;
    a.ist[I_NFEV] = nfev; a.ist[I_STATUS] = status;
    a.scale[0] = scale;
  }
}

// What run_evolve is asked for.  The objective: slot 0's posterior under an acquisition (model), or — model = nullptr — the debug
// walk's analytic sum (aw, aa, thresholds).
struct EvolveObjective {
  Model* model = nullptr;
  int acq = 0;
  double acq_param = 0.0, y_max = 0.0, y_mean = 0.0, y_std = 1.0;
  const double *aw = nullptr, *aa = nullptr;      // (D,) weights and targets
  double nan_below = 0.0, inf_above = 0.0;
};
// ... the space (column groups, bounds), the run (initial population, generations, the caller's MT19937 state) and where the result
// goes; or eval_n > 0 (debug): the objective at eval_n points, no run.
struct EvolveRun {
  int n_groups = 0;
  const int *kind = nullptr, *col0 = nullptr, *ncols = nullptr;
  const double *lo = nullptr, *hi = nullptr, *init = nullptr;
  int S = 0, D = 0, maxiter = 0;
  int budget = 0;      // evaluations per launch of the analytic objective (a model: the plan's): a launch ends at the first candidate boundary after them
  unsigned* key = nullptr;
  int* pos = nullptr;
  double *x_out = nullptr, *f_out = nullptr;
  int *nit_out = nullptr, *nfev_out = nullptr, *success_out = nullptr, *launches_out = nullptr;
  const double* eval_x = nullptr;
  int eval_n = 0;
  double* eval_out = nullptr;
};

struct DeviceBlock {      // freed on every way out
  char* p = nullptr;
  ~DeviceBlock() { (void)hipFree(p); }
};

// Device side of gpbo_evolve_mixed / the debug entries.
int run_evolve(gpbo_ctx* ctx, const EvolveObjective& o, const EvolveRun& r) {
  const int S = r.S, D = r.D, eval_n = r.eval_n;
  Model* const model = o.model;
  if (D < 1 || D > GPBO_MAX_DIM || S < 5 || S > EV_MAX_S || r.n_groups < 1 || r.n_groups > D || r.maxiter < 1 || (!model && r.budget < 1))
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: D in [1, 64], S in [5, 1024], maxiter >= 1 and one group per parameter");
  std::vector<int> ck(D, -1), cg0(D, 0), cgn(D, 1);
  for (int g = 0; g < r.n_groups; ++g) {
    if (r.kind[g] < 0 || r.kind[g] > 2 || r.ncols[g] < 1 || r.col0[g] < 0 || r.col0[g] + r.ncols[g] > D)
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: bad column group");
    for (int t = r.col0[g]; t < r.col0[g] + r.ncols[g]; ++t) {
      if (ck[t] >= 0) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: column groups overlap");
      ck[t] = r.kind[g]; cg0[t] = r.col0[g]; cgn[t] = r.ncols[g];
    }
  }
  for (int t = 0; t < D; ++t)
    if (ck[t] < 0) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: the column groups leave a column out");
  if (*r.pos < 0 || *r.pos > 624) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: MT19937 position outside [0, 624]");
  if (model) {
    if (!model->fitted || model->d != D) GPBO_FAIL(ctx, GPBO_ERR_STATE, "evolve: slot 0 is not fitted for this width");
    if (ctx->pending_info[0]) GPBO_FAIL(ctx, GPBO_ERR_STATE, "evolve: a fit of slot 0 is still in flight (gpbo_fit_wait)");
  }
  const int NP = model ? (int)model->NP : 0;
  const EvolvePlan plan = plan_evolve(NP, S, D, search_np_override(), !model);
  if (plan.mode == SearchMode::NotServed) {
    if (NP > search_max_np(search_np_override())) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "evolve: more than 512 (padded) observations");
    GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "evolve: the solver's state does not fit the LDS");
  }
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  // host-side scaling of SciPy's solver and the initial population
  std::vector<double> arg1(D), arg2(D), recip(D);
  for (int t = 0; t < D; ++t) {
    arg1[t] = 0.5 * (r.lo[t] + r.hi[t]);
    arg2[t] = std::fabs(r.lo[t] - r.hi[t]);
    const double rc = 1.0 / arg2[t];
    recip[t] = std::isfinite(rc) ? rc : 0.0;
  }
  // the run's block (search_plan.h): its host image, then the same layout over the device copy
  const EvolveBlock b = evolve_block(S, D, eval_n);
  std::vector<char> h(b.bytes);
  double* hd = (double*)h.data();
  int* hw = (int*)h.data();
  for (int s = 0; s < S; ++s)
    for (int t = 0; t < D; ++t) {
      const double u = (r.init ? (r.init[(size_t)s * D + t] - arg1[t]) * recip[t] + 0.5 : 0.0);
      hd[b.pop + (size_t)s * D + t] = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);      // np.clip: NaN stays NaN
    }
  for (int s = 0; s < S; ++s) { hd[b.E + s] = INFINITY; hw[b.perm + s] = s; }
  for (int t = 0; t < D; ++t) {
    hd[b.arg1 + t] = arg1[t]; hd[b.arg2 + t] = arg2[t];
    hd[b.aw + t] = o.aw ? o.aw[t] : 0.0; hd[b.aa + t] = o.aa ? o.aa[t] : 0.0;
    hw[b.ckind + t] = ck[t]; hw[b.cg0 + t] = cg0[t]; hw[b.cgn + t] = cgn[t];
  }
  if (eval_n) std::copy(r.eval_x, r.eval_x + (size_t)eval_n * D, hd + b.eval_x);
  hd[b.scale] = 0.0;
  int* h_ist = hw + b.ist;
  h_ist[I_POS] = *r.pos; h_ist[I_PHASE] = PH_PASS; h_ist[I_EV] = 0; h_ist[I_THEN] = PH_GEN; h_ist[I_C] = 0; h_ist[I_NIT] = 0;
  h_ist[I_NFEV] = 0; h_ist[I_STATUS] = 0;
  std::copy(r.key, r.key + 624, (unsigned*)(hw + b.key));
  DeviceBlock dblock;
  GPBO_HIP(ctx, hipMalloc(&dblock.p, b.bytes));
  GPBO_HIP(ctx, hipMemcpyAsync(dblock.p, h.data(), b.bytes, hipMemcpyHostToDevice, ctx->stream));
  double* dd = (double*)dblock.p;
  int* dw = (int*)dblock.p;
  EvolveArgs a{};
  a.analytic = model ? 0 : 1;
  a.amplitude = 1.0; a.white = 0.0;
  a.D = D; a.S = S; a.maxiter = r.maxiter; a.budget = model ? plan.evals_per_launch : r.budget;
  a.pop = dd + b.pop; a.energies = dd + b.E; a.arg1 = dd + b.arg1; a.arg2 = dd + b.arg2; a.aw = dd + b.aw; a.aa = dd + b.aa;
  a.eval_x = dd + b.eval_x; a.eval_out = dd + b.eval_out; a.scale = dd + b.scale;
  a.ist = dw + b.ist; a.perm = dw + b.perm; a.ckind = dw + b.ckind; a.cg0 = dw + b.cg0; a.cgn = dw + b.cgn;
  a.mt = (unsigned*)(dw + b.key);
  a.eval_n = eval_n;
  a.nan_below = o.nan_below; a.inf_above = o.inf_above;
  a.pop_lds = plan.pop_lds ? 1 : 0;
  a.acq = o.acq; a.acq_param = o.acq_param; a.y_max = o.y_max; a.y_mean = o.y_mean; a.y_std = o.y_std;
  dim3 block(64);
  if (model) {
    Model& m = *model;
    a.W = m.W; a.Xs = m.Xs; a.alpha = m.alpha; a.ls = m.ls;
    a.amplitude = m.amplitude; a.white = m.white;
    a.NP = NP; a.N = (int)m.N; a.DP = m.DP;
    block = dim3((unsigned)m.NP);
    if (plan.mode == SearchMode::WInMemory) {
      if (const int rc = ensure_w_transposed(ctx, m)) return rc;
      a.Wt = m.K;
    }
  }
  if (!(ctx->func_attrs & ATTR_EVOLVE)) {
    const int rc = for_each_kernel_wlds(ctx, [&](auto k, auto wlds) -> int {
      GPBO_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(evolve_kernel<decltype(k)::value, decltype(wlds)::value>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, SEARCH_LDS_BYTES));
      return GPBO_OK;
    });
    if (rc) return rc;
    ctx->func_attrs |= ATTR_EVOLVE;
  }
  int launches = 0;
  int st[I_COUNT];
  for (;;) {
    if (const int rc = with_kernel_wlds(ctx, model ? model->kernel : 0, plan.mode == SearchMode::WInLds, [&](auto k, auto wlds) -> int {
      evolve_kernel<decltype(k)::value, decltype(wlds)::value><<<dim3(1), block, (size_t)plan.lds_bytes, ctx->stream>>>(a);
      return GPBO_OK;
    })) return rc;
    ++launches;
    GPBO_HIP(ctx, hipGetLastError());
    GPBO_HIP(ctx, hipMemcpyAsync(st, a.ist, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    GPBO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (eval_n > 0 || st[I_PHASE] == PH_DONE) break;
  }
  GPBO_HIP(ctx, hipMemcpy(h.data(), dblock.p, b.bytes, hipMemcpyDeviceToHost));
  if (r.launches_out) *r.launches_out = launches;
  if (eval_n > 0) {
    std::copy(hd + b.eval_out, hd + b.eval_out + eval_n, r.eval_out);
    return GPBO_OK;
  }
  std::copy((unsigned*)(hw + b.key), (unsigned*)(hw + b.key) + 624, r.key);
  *r.pos = h_ist[I_POS];
  for (int t = 0; t < D; ++t) r.x_out[t] = arg1[t] + (hd[b.pop + t] - 0.5) * arg2[t];
  *r.f_out = hd[b.E];
  *r.nit_out = h_ist[I_NIT];
  *r.nfev_out = h_ist[I_NFEV];
  *r.success_out = h_ist[I_STATUS] == 1 ? 1 : 0;
  return GPBO_OK;
}

}  // namespace

}  // namespace gpbo

using namespace gpbo;

extern "C" int gpbo_evolve_mixed(gpbo_ctx* ctx, int acq, double acq_param, double y_max, double y_mean, double y_std, int n_groups,
                                 const int* kind, const int* col0, const int* ncols, const double* bounds_lo, const double* bounds_hi,
                                 const double* init, int S, int D, int maxiter, unsigned* key, int* pos, double* x_out, double* f_out,
                                 int* nit_out, int* nfev_out, int* success_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!kind || !col0 || !ncols || !bounds_lo || !bounds_hi || !init || !key || !pos || !x_out || !f_out || !nit_out || !nfev_out ||
      !success_out)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve_mixed: NULL argument");
  if (acq == GPBO_ACQ_LOG_EI) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve_mixed: GPBO_ACQ_LOG_EI is not evaluated by the device differential evolution");
  if (acq == GPBO_ACQ_LOG_CEI) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve_mixed: GPBO_ACQ_LOG_CEI is not evaluated by the device differential evolution");
  if (acq == GPBO_ACQ_LOG_FEAS) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve_mixed: GPBO_ACQ_LOG_FEAS is not evaluated by the device differential evolution (it takes no constraints)");
  if (acq != GPBO_ACQ_UCB && acq != GPBO_ACQ_EI && acq != GPBO_ACQ_POI) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve_mixed: unknown acquisition");
  drop_refreshable(ctx);      // as gpbo_polish_seeds: nothing resident may be refreshed after a search
  EvolveObjective o;
  o.model = &ctx->models[0];
  o.acq = acq; o.acq_param = acq_param; o.y_max = y_max; o.y_mean = y_mean; o.y_std = y_std;
  EvolveRun r;
  r.n_groups = n_groups; r.kind = kind; r.col0 = col0; r.ncols = ncols;
  r.lo = bounds_lo; r.hi = bounds_hi; r.init = init;
  r.S = S; r.D = D; r.maxiter = maxiter;
  r.key = key; r.pos = pos;
  r.x_out = x_out; r.f_out = f_out; r.nit_out = nit_out; r.nfev_out = nfev_out; r.success_out = success_out;
  return run_evolve(ctx, o, r);
}

#ifdef GPBO_DEBUG
extern "C" int gpbo_debug_evolve_eval(gpbo_ctx* ctx, int acq, double acq_param, double y_max, double y_mean, double y_std, int n_groups,
                                      const int* kind, const int* col0, const int* ncols, const double* points, int n, int D,
                                      double* out) {
  if (!ctx || !kind || !col0 || !ncols || !points || !out || n < 1) return GPBO_ERR_INVALID;
  std::vector<double> lo(D, 0.0), hi(D, 1.0);
  unsigned key[624] = {};
  int pos = 624;
  EvolveObjective o;
  o.model = &ctx->models[0];
  o.acq = acq; o.acq_param = acq_param; o.y_max = y_max; o.y_mean = y_mean; o.y_std = y_std;
  EvolveRun r;      // the smallest legal run around the points: nothing of it is stepped
  r.n_groups = n_groups; r.kind = kind; r.col0 = col0; r.ncols = ncols;
  r.lo = lo.data(); r.hi = hi.data();
  r.S = 5; r.D = D; r.maxiter = 1;
  r.key = key; r.pos = &pos;
  r.eval_x = points; r.eval_n = n; r.eval_out = out;
  return run_evolve(ctx, o, r);
}

extern "C" int gpbo_debug_evolve_walk(gpbo_ctx* ctx, const double* weights, const double* targets, double nan_below, double inf_above,
                                      int n_groups, const int* kind, const int* col0, const int* ncols, const double* bounds_lo,
                                      const double* bounds_hi, const double* init, int S, int D, int maxiter, int budget, unsigned* key,
                                      int* pos, double* x_out, double* f_out, int* nit_out, int* nfev_out, int* success_out,
                                      int* launches_out) {
  if (!ctx || !weights || !targets || !kind || !col0 || !ncols || !bounds_lo || !bounds_hi || !init || !key || !pos || !x_out ||
      !f_out || !nit_out || !nfev_out || !success_out)
    return GPBO_ERR_INVALID;
  EvolveObjective o;
  o.aw = weights; o.aa = targets; o.nan_below = nan_below; o.inf_above = inf_above;
  EvolveRun r;
  r.n_groups = n_groups; r.kind = kind; r.col0 = col0; r.ncols = ncols;
  r.lo = bounds_lo; r.hi = bounds_hi; r.init = init;
  r.S = S; r.D = D; r.maxiter = maxiter; r.budget = budget;
  r.key = key; r.pos = pos;
  r.x_out = x_out; r.f_out = f_out; r.nit_out = nit_out; r.nfev_out = nfev_out; r.success_out = success_out; r.launches_out = launches_out;
  return run_evolve(ctx, o, r);
}
#endif  // GPBO_DEBUG
