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
// NP <= 128 when it fits, its transposed copy streamed from memory up to 512), then -base_acq(mu, sd) with the acquisition kernels'
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

constexpr int EV_LDS_NP = 128;           // W in LDS up to here (when it fits beside the solver's state)
constexpr int EV_MAX_NP = 512;
constexpr int EV_MAX_S = 1024;
constexpr size_t EV_LDS_CAP = 160 * 1024;

enum EvPhase { PH_PASS = 0, PH_GEN = 1, PH_SCALE = 2, PH_CAND = 3, PH_DONE = 4 };
// integer state words in device memory
enum EvInt { I_POS = 0, I_PHASE, I_EV, I_THEN, I_C, I_NIT, I_NFEV, I_STATUS, I_COUNT = 8 };

struct EvolveArgs {
  // objective: slot 0's posterior (analytic = 0) or the debug walk's analytic sum (analytic = 1)
  const double *W, *Wt, *Xs, *alpha, *ls;
  int NP, N, DP;
  double y_mean, y_std;
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

__device__ __forceinline__ double ev_lane(double v, int i) {      // v of lane i (i uniform), in every lane
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), i);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), i);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
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
    const double v = ev_lane(bv, l);
    if (bn >= 0 && (gnan < 0 || bn < gnan)) gnan = bn;
    if (bi >= 0 && (gbest < 0 || v < gv || (v == gv && bi < gbest))) { gbest = bi; gv = v; }
  }
  return gnan >= 0 ? gnan : (gbest >= 0 ? gbest : 0);
}

// NumPy's pairwise float64 sum of f(E[i]) (8 accumulators up to 128 values, halves above), uniform over wave 0.  The recursion runs
// on an explicit stack in LDS (frames: lo, n, state; partial sums), post-order: left half, right half, left + right.
constexpr int EV_STACK = 16;
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
__global__ __launch_bounds__(EV_MAX_NP) void evolve_kernel(const EvolveArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double ev_smem[];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int NP = a.analytic ? 0 : a.NP, N = a.N, D = a.D, S = a.S, DP = a.DP;
  const int WLD = NP + 1;
  double* Wl = ev_smem;
  double* xs = Wl + (WLDS ? NP * WLD : 0);   // [64]
  double* ls_s = xs + 64;                    // [64]
  double* px = ls_s + 64;                    // [64] the point in parameter space
  double* ks = px + 64;                      // [NP]
  double* vs = ks + NP;                      // [NP]
  double* pp = vs + NP;                      // [2 NP]
  double* E = pp + 2 * NP;                   // [S]
  double* misc = E + S;                      // [8]: [0] the energy, [1] stop flag
  double* stk_acc = misc + 8;                // [EV_STACK] partial sums of the pairwise summation
  double* popl = stk_acc + EV_STACK;         // [S][D] when the population fits
  unsigned* key = (unsigned*)(popl + (a.pop_lds ? (size_t)S * D : 0));      // [624]
  int* perm = (int*)(key + 624);             // [S]
  int* frames = perm + S;                    // [EV_STACK][3] its frames
  double* pop = a.pop_lds ? popl : a.pop;

  if (!a.analytic) {
    if (WLDS)
      for (int e = tid; e < NP * NP; e += NP) {
        const int i = e / NP, k = e - i * NP;
        Wl[i * WLD + k] = a.W[e];
      }
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
      s2 = ev_lane(s2, 0);
      mm = ev_lane(mm, 0);
      double var = 1.0 - s2;
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

size_t ev_lds_bytes(int NP, int S, int D, bool wlds, bool pop_lds) {
  return ((size_t)(wlds ? NP * (NP + 1) : 0) + 192 + 4 * (size_t)NP + S + 8 + EV_STACK + (pop_lds ? (size_t)S * D : 0)) * sizeof(double) +
         (624 + (size_t)S + 3 * EV_STACK) * sizeof(int);
}

}  // namespace

// Device side of gpbo_evolve_mixed / the debug entries.  model = nullptr: the analytic objective (aw, aa, thresholds).
// Evaluations per launch: a launch ends at the first candidate boundary after `budget` of them.
int run_evolve(gpbo_ctx* ctx, Model* model, int acq, double acq_param, double y_max, double y_mean, double y_std, const double* aw,
               const double* aa, double nan_below, double inf_above, int n_groups, const int* kind, const int* col0, const int* ncols,
               const double* lo, const double* hi, const double* init, int S, int D, int maxiter, int budget, unsigned* key, int* pos,
               double* x_out, double* f_out, int* nit_out, int* nfev_out, int* success_out, const double* eval_x, int eval_n,
               double* eval_out, int* launches_out) {
  if (D < 1 || D > GPBO_MAX_DIM || S < 5 || S > EV_MAX_S || n_groups < 1 || n_groups > D || maxiter < 1 || budget < 1)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: D in [1, 64], S in [5, 1024], maxiter >= 1 and one group per parameter");
  std::vector<int> ck(D, -1), cg0(D, 0), cgn(D, 1);
  for (int g = 0; g < n_groups; ++g) {
    if (kind[g] < 0 || kind[g] > 2 || ncols[g] < 1 || col0[g] < 0 || col0[g] + ncols[g] > D)
      GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: bad column group");
    for (int t = col0[g]; t < col0[g] + ncols[g]; ++t) {
      if (ck[t] >= 0) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: column groups overlap");
      ck[t] = kind[g]; cg0[t] = col0[g]; cgn[t] = ncols[g];
    }
  }
  for (int t = 0; t < D; ++t)
    if (ck[t] < 0) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: the column groups leave a column out");
  if (*pos < 0 || *pos > 624) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve: MT19937 position outside [0, 624]");
  int mode = 0;      // 1: W in LDS, 2: W in memory
  bool pop_lds = false;
  if (model) {
    Model& m = *model;
    if (!m.fitted || m.d != D) GPBO_FAIL(ctx, GPBO_ERR_STATE, "evolve: slot 0 is not fitted for this width");
    if (ctx->pending_info[0]) GPBO_FAIL(ctx, GPBO_ERR_STATE, "evolve: a fit of slot 0 is still in flight (gpbo_fit_wait)");
    if (m.NP > EV_MAX_NP || m.NP > polish_fused_max_np()) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "evolve: more than 512 (padded) observations");
    pop_lds = ev_lds_bytes((int)m.NP, S, D, m.NP <= EV_LDS_NP, true) <= EV_LDS_CAP;
    if (m.NP <= EV_LDS_NP && ev_lds_bytes((int)m.NP, S, D, true, pop_lds) <= EV_LDS_CAP) mode = 1;
    else {
      pop_lds = ev_lds_bytes((int)m.NP, S, D, false, true) <= EV_LDS_CAP;
      if (ev_lds_bytes((int)m.NP, S, D, false, pop_lds) <= EV_LDS_CAP) mode = 2;
    }
    if (!mode) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "evolve: the solver's state does not fit the LDS");
  } else {
    pop_lds = ev_lds_bytes(0, S, D, false, true) <= EV_LDS_CAP;
  }
  GPBO_HIP(ctx, hipSetDevice(ctx->device));
  // host-side scaling of SciPy's solver and the initial population
  std::vector<double> arg1(D), arg2(D), recip(D);
  for (int t = 0; t < D; ++t) {
    arg1[t] = 0.5 * (lo[t] + hi[t]);
    arg2[t] = std::fabs(lo[t] - hi[t]);
    const double r = 1.0 / arg2[t];
    recip[t] = std::isfinite(r) ? r : 0.0;
  }
  // device block: doubles [pop S D | E S | arg1 D | arg2 D | aw D | aa D | eval_x | eval_out | scale] then ints [ist 8 | perm S | ck D |
  // cg0 D | cgn D] then the key
  const size_t nd = (size_t)S * D + S + 4 * (size_t)D + (size_t)eval_n * D + eval_n + 1;
  const size_t ni = I_COUNT + (size_t)S + 3 * (size_t)D + 624;
  const size_t bytes = nd * sizeof(double) + ni * sizeof(int);
  std::vector<char> h(bytes);
  double* hd = (double*)h.data();
  double* h_pop = hd;
  double* h_E = h_pop + (size_t)S * D;
  double* h_a1 = h_E + S;
  double* h_a2 = h_a1 + D;
  double* h_aw = h_a2 + D;
  double* h_aa = h_aw + D;
  double* h_ex = h_aa + D;
  double* h_eo = h_ex + (size_t)eval_n * D;
  double* h_sc = h_eo + eval_n;
  int* hi_ = (int*)(hd + nd);
  int* h_ist = hi_;
  int* h_perm = h_ist + I_COUNT;
  int* h_ck = h_perm + S;
  int* h_cg0 = h_ck + D;
  int* h_cgn = h_cg0 + D;
  unsigned* h_key = (unsigned*)(h_cgn + D);
  for (int s = 0; s < S; ++s)
    for (int t = 0; t < D; ++t) {
      const double u = (init ? (init[(size_t)s * D + t] - arg1[t]) * recip[t] + 0.5 : 0.0);
      h_pop[(size_t)s * D + t] = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);      // np.clip: NaN stays NaN
    }
  for (int s = 0; s < S; ++s) { h_E[s] = INFINITY; h_perm[s] = s; }
  for (int t = 0; t < D; ++t) {
    h_a1[t] = arg1[t]; h_a2[t] = arg2[t];
    h_aw[t] = aw ? aw[t] : 0.0; h_aa[t] = aa ? aa[t] : 0.0;
    h_ck[t] = ck[t]; h_cg0[t] = cg0[t]; h_cgn[t] = cgn[t];
  }
  if (eval_n) std::copy(eval_x, eval_x + (size_t)eval_n * D, h_ex);
  h_sc[0] = 0.0;
  h_ist[I_POS] = *pos; h_ist[I_PHASE] = PH_PASS; h_ist[I_EV] = 0; h_ist[I_THEN] = PH_GEN; h_ist[I_C] = 0; h_ist[I_NIT] = 0;
  h_ist[I_NFEV] = 0; h_ist[I_STATUS] = 0;
  std::copy(key, key + 624, h_key);
  char* dblock = nullptr;
  GPBO_HIP(ctx, hipMalloc(&dblock, bytes));
  auto release = [&]() { (void)hipFree(dblock); };
  {
    hipError_t e = hipMemcpyAsync(dblock, h.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) { release(); GPBO_HIP(ctx, e); }
  }
  double* dd = (double*)dblock;
  int* di = (int*)(dd + nd);
  EvolveArgs a{};
  a.analytic = model ? 0 : 1;
  a.D = D; a.S = S; a.maxiter = maxiter; a.budget = budget;
  a.pop = dd; a.energies = dd + (size_t)S * D; a.arg1 = a.energies + S; a.arg2 = a.arg1 + D; a.aw = a.arg2 + D; a.aa = a.aw + D;
  a.eval_x = a.aa + D; a.eval_out = (double*)a.eval_x + (size_t)eval_n * D; a.scale = a.eval_out + eval_n;
  a.ist = di; a.perm = di + I_COUNT; a.ckind = a.perm + S; a.cg0 = a.ckind + D; a.cgn = a.cg0 + D;
  a.mt = (unsigned*)(a.cgn + D);
  a.eval_n = eval_n;
  a.nan_below = nan_below; a.inf_above = inf_above;
  a.pop_lds = pop_lds ? 1 : 0;
  a.acq = acq; a.acq_param = acq_param; a.y_max = y_max; a.y_mean = y_mean; a.y_std = y_std;
  size_t lds;
  dim3 block(64);
  int kern = 0;
  if (model) {
    Model& m = *model;
    a.W = m.W; a.Xs = m.Xs; a.alpha = m.alpha; a.ls = m.ls;
    a.NP = (int)m.NP; a.N = (int)m.N; a.DP = m.DP;
    kern = m.kernel;
    block = dim3((unsigned)m.NP);
    if (mode == 2) {
      int rc = ensure_w_transposed(ctx, m);
      if (rc) { release(); return rc; }
      a.Wt = m.K;
    }
    lds = ev_lds_bytes((int)m.NP, S, D, mode == 1, pop_lds);
  } else {
    a.DP = 0;
    lds = ev_lds_bytes(0, S, D, false, pop_lds);
  }
  if (!(ctx->func_attrs & ATTR_EVOLVE)) {
    const void* ks[4] = {reinterpret_cast<const void*>(evolve_kernel<GPBO_KERNEL_MATERN25, true>),
                         reinterpret_cast<const void*>(evolve_kernel<GPBO_KERNEL_RBF, true>),
                         reinterpret_cast<const void*>(evolve_kernel<GPBO_KERNEL_MATERN25, false>),
                         reinterpret_cast<const void*>(evolve_kernel<GPBO_KERNEL_RBF, false>)};
    for (const void* k : ks) {
      hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)EV_LDS_CAP);
      if (e != hipSuccess) { release(); GPBO_HIP(ctx, e); }
    }
    ctx->func_attrs |= ATTR_EVOLVE;
  }
  int launches = 0;
  int st[I_COUNT];
  for (;;) {
    if (mode == 1) {
      if (kern == GPBO_KERNEL_MATERN25) evolve_kernel<GPBO_KERNEL_MATERN25, true><<<dim3(1), block, lds, ctx->stream>>>(a);
      else evolve_kernel<GPBO_KERNEL_RBF, true><<<dim3(1), block, lds, ctx->stream>>>(a);
    } else {
      if (kern == GPBO_KERNEL_MATERN25) evolve_kernel<GPBO_KERNEL_MATERN25, false><<<dim3(1), block, lds, ctx->stream>>>(a);
      else evolve_kernel<GPBO_KERNEL_RBF, false><<<dim3(1), block, lds, ctx->stream>>>(a);
    }
    ++launches;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(st, di, sizeof(st), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { release(); GPBO_HIP(ctx, e); }
    if (eval_n > 0 || st[I_PHASE] == PH_DONE) break;
  }
  {
    hipError_t e = hipMemcpy(h.data(), dblock, bytes, hipMemcpyDeviceToHost);
    release();
    GPBO_HIP(ctx, e);
  }
  if (launches_out) *launches_out = launches;
  if (eval_n > 0) {
    std::copy(h_eo, h_eo + eval_n, eval_out);
    return GPBO_OK;
  }
  std::copy(h_key, h_key + 624, key);
  *pos = h_ist[I_POS];
  for (int t = 0; t < D; ++t) x_out[t] = arg1[t] + (h_pop[t] - 0.5) * arg2[t];
  *f_out = h_E[0];
  *nit_out = h_ist[I_NIT];
  *nfev_out = h_ist[I_NFEV];
  *success_out = h_ist[I_STATUS] == 1 ? 1 : 0;
  return GPBO_OK;
}

}  // namespace gpbo

using namespace gpbo;

namespace {
// Evaluations per launch: ~2 ms of work at the per-evaluation cost of each size band (3-6 us up to NP = 128, 16-41 us up to 512)
int evolve_budget(const Model& m) { return m.NP <= 128 ? 384 : (m.NP <= 256 ? 96 : 48); }
}  // namespace

extern "C" int gpbo_evolve_mixed(gpbo_ctx* ctx, int acq, double acq_param, double y_max, double y_mean, double y_std, int n_groups,
                                 const int* kind, const int* col0, const int* ncols, const double* bounds_lo, const double* bounds_hi,
                                 const double* init, int S, int D, int maxiter, unsigned* key, int* pos, double* x_out, double* f_out,
                                 int* nit_out, int* nfev_out, int* success_out) {
  if (!ctx) return GPBO_ERR_INVALID;
  if (!kind || !col0 || !ncols || !bounds_lo || !bounds_hi || !init || !key || !pos || !x_out || !f_out || !nit_out || !nfev_out ||
      !success_out)
    GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve_mixed: NULL argument");
  if (acq != GPBO_ACQ_UCB && acq != GPBO_ACQ_EI && acq != GPBO_ACQ_POI) GPBO_FAIL(ctx, GPBO_ERR_INVALID, "evolve_mixed: unknown acquisition");
  Model& m = ctx->models[0];
  return run_evolve(ctx, &m, acq, acq_param, y_max, y_mean, y_std, nullptr, nullptr, 0.0, 0.0, n_groups, kind, col0, ncols, bounds_lo,
                    bounds_hi, init, S, D, maxiter, m.fitted ? evolve_budget(m) : 1, key, pos, x_out, f_out, nit_out, nfev_out,
                    success_out, nullptr, 0, nullptr, nullptr);
}

#ifdef GPBO_DEBUG
extern "C" int gpbo_debug_evolve_eval(gpbo_ctx* ctx, int acq, double acq_param, double y_max, double y_mean, double y_std, int n_groups,
                                      const int* kind, const int* col0, const int* ncols, const double* points, int n, int D,
                                      double* out) {
  if (!ctx || !kind || !col0 || !ncols || !points || !out || n < 1) return GPBO_ERR_INVALID;
  std::vector<double> lo(D, 0.0), hi(D, 1.0);
  unsigned key[624] = {};
  int pos = 624, nit = 0, nfev = 0, ok = 0;
  double x[GPBO_MAX_DIM], f;
  Model& m = ctx->models[0];
  return run_evolve(ctx, &m, acq, acq_param, y_max, y_mean, y_std, nullptr, nullptr, 0.0, 0.0, n_groups, kind, col0, ncols, lo.data(),
                    hi.data(), nullptr, 5, D, 1, 1, key, &pos, x, &f, &nit, &nfev, &ok, points, n, out, nullptr);
}

extern "C" int gpbo_debug_evolve_walk(gpbo_ctx* ctx, const double* weights, const double* targets, double nan_below, double inf_above,
                                      int n_groups, const int* kind, const int* col0, const int* ncols, const double* bounds_lo,
                                      const double* bounds_hi, const double* init, int S, int D, int maxiter, int budget, unsigned* key,
                                      int* pos, double* x_out, double* f_out, int* nit_out, int* nfev_out, int* success_out,
                                      int* launches_out) {
  if (!ctx || !weights || !targets || !kind || !col0 || !ncols || !bounds_lo || !bounds_hi || !init || !key || !pos || !x_out ||
      !f_out || !nit_out || !nfev_out || !success_out)
    return GPBO_ERR_INVALID;
  return run_evolve(ctx, nullptr, 0, 0.0, 0.0, 0.0, 1.0, weights, targets, nan_below, inf_above, n_groups, kind, col0, ncols, bounds_lo,
                    bounds_hi, init, S, D, maxiter, budget, key, pos, x_out, f_out, nit_out, nfev_out, success_out, nullptr, 0, nullptr,
                    launches_out);
}
#endif  // GPBO_DEBUG
