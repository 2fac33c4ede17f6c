// How the one-launch searches are served and laid out, as pure functions of plain values: gpbo_polish_seeds' local searches
// (polish_fused.hip: polish_rows_kernel) and gpbo_evolve_mixed's differential evolution (evolve.hip: evolve_kernel).  Both evaluate
// the posterior with a thread per training point (posterior_rows.h), so they share one serve rule: W in LDS, W streamed from
// memory, or not served.  Here too: each kernel's LDS layout (the kernel takes its pointers from it, the host its dynamic-LDS byte
// count) and the layout of each host / device block (applied to the host address by the readers, to the device address by the
// launcher).  Free of HIP: tests/test_search_plan_host.py compiles it with the system C++ compiler and pins the rule on both sides
// of every edge.  The debug switches (GPBO_POLISH_FUSED, GPBO_POLISH_FUSED_MAX_NP) are read by the caller and come in already
// fetched / parsed (NO_OVERRIDE: not set).
#pragma once

#include <algorithm>
#include <cstddef>

#include "fit_plan.h"   // NO_OVERRIDE

#ifdef __HIPCC__
#define GPBO_PLAN_HD __host__ __device__ inline
#else
#define GPBO_PLAN_HD inline
#endif

namespace gpbo {

constexpr int SEARCH_LDS_NP = 128;       // W fits the LDS up to here (a padded square [NP][NP + 1]: 132 KB at 128)
constexpr int SEARCH_MAX_NP = 512;       // ... and is streamed from memory above (W for the column walk, its transpose for the row walk): 8 waves,
                                         // 256 VGPRs each (12 waves for NP = 768 would spill the optimiser's registers to scratch)
// Served up to this padded size, one model — the kernels' own limit: at N = 512 the launch still beats the lockstep rounds
// (profiles/r06_polish_fused_ab.json: 0.36-0.48 against 0.53-0.59 ms for 8-10 evaluations, 2.09 against 2.13 for 48)
constexpr int SEARCH_NP_DEFAULT = 512;
constexpr int SEARCH_LDS_BYTES = 160 * 1024;
constexpr int POLISH_X_CAP = SEARCH_LDS_BYTES / 8 - 8;      // doubles in 160 KiB, less the flag words: X is staged when it fits below this
constexpr int POLISH_OPT_PAIRS = 10;     // polish_opt.h's LBFGS_M (polish_fused.hip asserts it)
constexpr int EV_MAX_S = 1024;           // largest population of the evolution
constexpr int EV_STACK = 16;             // frames of the pairwise summation's explicit stack (evolve.hip: ev_pairwise)

enum class SearchMode { NotServed = 0, WInLds = 1, WInMemory = 2 };

// Largest padded size both searches serve.  Debug build: GPBO_POLISH_FUSED_MAX_NP, read per call — the crossover against the lockstep
// rounds, scripts/r06_polish_fused_ab.py: at N = 512 a run of ~50 evaluations already loses to them, 2.46 against 2.13 ms — and
// 0 = never, the lockstep path alone: the checker's switch, with GPBO_POLISH_FUSED=0.  The evolution has no other path: above
// this size it reports GPBO_ERR_UNSUPPORTED, so the switch moves its limit too.
inline int search_max_np(int override) { return std::min(override == NO_OVERRIDE ? SEARCH_NP_DEFAULT : override, SEARCH_MAX_NP); }

// ---- polish_rows_kernel ---------------------------------------------------------------------------------------------------------
// the sums over the training points are taken by lane groups of DP lanes, one dimension each
GPBO_PLAN_HD int polish_groups(int NP, int DP) { return (64 / DP) * (NP >> 6); }
// the optimiser's block: S, Y [pairs][d] (lane i reads and writes column i) | s.y, y.y over ALL variables, rho, a [pairs each]
// (written and read by every lane alike: program order within the one wave)
GPBO_PLAN_HD int polish_opt_doubles(int d) { return 2 * POLISH_OPT_PAIRS * d + 4 * POLISH_OPT_PAIRS; }

// Dynamic LDS of polish_rows_kernel: offsets in doubles, in this order, nothing between the arrays.
struct PolishLds {
  int W;        // [NP][NP + 1] (WLDS): row walks and column walks both hit 64 different banks
  int xs;       // [64] the trial point over the length scales, zero padded
  int ls;       // [64]
  int alpha;    // [NP]
  int ks;       // [NP] k*
  int vs;       // [NP] v = W k*
  int cc;       // [NP][2] alpha_k f_k, u_k f_k
  int pp;       // [NP][2] v_k^2, k*_k alpha_k
  int us;       // [NP] u = W^T v (W in memory: the pair threads hand their columns' sums over)
  int red;      // [groups][2 DP + 2] group partials
  int opt;      // polish_opt_doubles(d)
  int X;        // [NP][DP + 1] the scaled inputs, when they fit (x_doubles of them, else 0)
  int x_doubles;
  int flag;     // two ints: the stop flag
  int bytes;
};
GPBO_PLAN_HD PolishLds polish_lds(int NP, int d, int DP, bool wlds) {
  PolishLds l{};
  l.W = 0;
  l.xs = l.W + (wlds ? NP * (NP + 1) : 0);
  l.ls = l.xs + 64;
  l.alpha = l.ls + 64;
  l.ks = l.alpha + NP;
  l.vs = l.ks + NP;
  l.cc = l.vs + NP;
  l.pp = l.cc + 2 * NP;
  l.us = l.pp + 2 * NP;
  l.red = l.us + NP;
  l.opt = l.red + polish_groups(NP, DP) * (2 * DP + 2);
  l.X = l.opt + polish_opt_doubles(d);
  const int want = NP * (DP + 1);
  l.x_doubles = (l.X + want <= POLISH_X_CAP) ? want : 0;
  l.flag = l.X + l.x_doubles;
  l.bytes = l.flag * 8 + 16;
  return l;
}

struct PolishPlan {
  SearchMode mode;
  int lds_bytes;
  bool x_staged;
};
// W in LDS for NP <= 128, streamed from memory up to the cap.  By polish_lds both images fit for every d <= 64 with its pad_dim
// even before X is staged: the largest W-in-LDS image (NP = 128, d = DP = 64) needs 19 244 of the 20 478 doubles that 160 KiB
// less the flag words hold, the largest streamed one (NP = 512) 6 584 — "does not fit" cannot happen today; the check stays for
// the array that is added tomorrow (tests/test_search_plan_host.py holds the two figures).
inline PolishPlan plan_polish(int NP, int d, int DP, int max_np_override) {
  if (NP <= search_max_np(max_np_override))
    for (const SearchMode mode : {SearchMode::WInLds, SearchMode::WInMemory}) {
      const PolishLds l = polish_lds(NP, d, DP, mode == SearchMode::WInLds);
      if (NP <= (mode == SearchMode::WInLds ? SEARCH_LDS_NP : SEARCH_MAX_NP) && l.bytes <= SEARCH_LDS_BYTES)
        return {mode, l.bytes, l.x_doubles != 0};
    }
  return {SearchMode::NotServed, 0, false};
}

// gpbo_polish_seeds runs its searches as the one launch for one model that the plan serves, unless GPBO_POLISH_FUSED (debug build)
// starts with '0'
inline bool polish_one_launch(int n_constraints, SearchMode mode, const char* fused_switch) {
  return n_constraints == 0 && mode != SearchMode::NotServed && !(fused_switch && fused_switch[0] == '0');
}

// The pinned block (device-visible) of the one launch: doubles [seeds (S, d) | lo (d) | hi (d) | x (S, d) | f (S) | dbg (S, 4 + 3 d)]
// then ints [status (S) | iter (S) | evals (S)].  Offsets in doubles / in ints from the block's start.
struct PolishBlock {
  size_t seeds, lo, hi, x, f, dbg, ints;      // (ints: where the doubles end)
  size_t status, iter, evals;
  size_t bytes;
};
inline PolishBlock polish_block(int n_seeds, int d) {
  const size_t S = (size_t)n_seeds, D = (size_t)d;
  PolishBlock b{};
  b.seeds = 0;
  b.lo = b.seeds + S * D;
  b.hi = b.lo + D;
  b.x = b.hi + D;
  b.f = b.x + S * D;
  b.dbg = b.f + S;
  b.ints = b.dbg + S * (4 + 3 * D);
  b.status = 2 * b.ints;
  b.iter = b.status + S;
  b.evals = b.iter + S;
  b.bytes = (b.evals + S) * sizeof(int);
  return b;
}

// ---- evolve_kernel --------------------------------------------------------------------------------------------------------------
// Dynamic LDS of evolve_kernel: the double arrays (offsets in doubles) then the int arrays (offsets in ints), in this order.  NP = 0:
// the analytic objective of the debug walk (no posterior arrays).
struct EvolveLds {
  int W;        // [NP][NP + 1] (WLDS)
  int xs;       // [64]
  int ls;       // [64]
  int px;       // [64] the point in parameter space
  int ks;       // [NP]
  int vs;       // [NP]
  int pp;       // [2 NP]
  int E;        // [S] energies
  int misc;     // [8]: [0] the energy, [1] stop flag
  int acc;      // [EV_STACK] partial sums of the pairwise summation
  int pop;      // [S][D] when the population fits
  int key;      // ints from here: [624] MT19937 words
  int perm;     // [S]
  int frames;   // [EV_STACK][3]
  int bytes;
};
GPBO_PLAN_HD EvolveLds evolve_lds(int NP, int S, int D, bool wlds, bool pop_lds) {
  EvolveLds l{};
  l.W = 0;
  l.xs = l.W + (wlds ? NP * (NP + 1) : 0);
  l.ls = l.xs + 64;
  l.px = l.ls + 64;
  l.ks = l.px + 64;
  l.vs = l.ks + NP;
  l.pp = l.vs + NP;
  l.E = l.pp + 2 * NP;
  l.misc = l.E + S;
  l.acc = l.misc + 8;
  l.pop = l.acc + EV_STACK;
  l.key = 2 * (l.pop + (pop_lds ? S * D : 0));
  l.perm = l.key + 624;
  l.frames = l.perm + S;
  l.bytes = (l.frames + 3 * EV_STACK) * 4;
  return l;
}

struct EvolvePlan {
  SearchMode mode;       // analytic: NotServed is never returned — no W at all, the kernel runs its WLDS = false instance
  bool pop_lds;          // the population sits in LDS during a launch (else it stays in device memory)
  int lds_bytes;
  int evals_per_launch;  // ~2 ms of work at the per-evaluation cost of each size band (3-6 us up to NP = 128, 16-41 us up to 512)
};
// The population joins W in LDS when both fit; W in LDS without the population comes before W in memory with it.  The analytic
// objective has no model: NP = 0 whatever the caller holds, no size cap, and with S <= EV_MAX_S its state always fits.
inline EvolvePlan plan_evolve(int NP, int S, int D, int max_np_override, bool analytic) {
  if (analytic) NP = 0;
  const int budget = NP <= 128 ? 384 : (NP <= 256 ? 96 : 48);
  const bool w_may_sit_in_lds = !analytic && NP <= SEARCH_LDS_NP;
  if (analytic || NP <= search_max_np(max_np_override))
    for (const bool wlds : {true, false}) {
      if (wlds && !w_may_sit_in_lds) continue;
      const bool pop = evolve_lds(NP, S, D, wlds, true).bytes <= SEARCH_LDS_BYTES;
      const int bytes = evolve_lds(NP, S, D, wlds, pop).bytes;
      if (bytes <= SEARCH_LDS_BYTES) return {wlds ? SearchMode::WInLds : SearchMode::WInMemory, pop, bytes, budget};
    }
  return {SearchMode::NotServed, false, 0, budget};
}

// integer state words of the evolution in device memory
enum EvInt { I_POS = 0, I_PHASE, I_EV, I_THEN, I_C, I_NIT, I_NFEV, I_STATUS, I_COUNT = 8 };
// The device block of a run and its host image: doubles [pop S D | E S | arg1 D | arg2 D | aw D | aa D | eval_x | eval_out | scale]
// then ints [ist I_COUNT | perm S | ckind D | cg0 D | cgn D | the MT19937 key 624].  Offsets in doubles / in ints from the start.
struct EvolveBlock {
  size_t pop, E, arg1, arg2, aw, aa, eval_x, eval_out, scale, ints;      // (ints: where the doubles end)
  size_t ist, perm, ckind, cg0, cgn, key;
  size_t bytes;
};
inline EvolveBlock evolve_block(int S_, int D_, int eval_n) {
  const size_t S = (size_t)S_, D = (size_t)D_, n = (size_t)eval_n;
  EvolveBlock b{};
  b.pop = 0;
  b.E = b.pop + S * D;
  b.arg1 = b.E + S;
  b.arg2 = b.arg1 + D;
  b.aw = b.arg2 + D;
  b.aa = b.aw + D;
  b.eval_x = b.aa + D;
  b.eval_out = b.eval_x + n * D;
  b.scale = b.eval_out + n;
  b.ints = b.scale + 1;
  b.ist = 2 * b.ints;
  b.perm = b.ist + I_COUNT;
  b.ckind = b.perm + S;
  b.cg0 = b.ckind + D;
  b.cgn = b.cg0 + D;
  b.key = b.cgn + D;
  b.bytes = (b.key + 624) * sizeof(int);
  return b;
}

}  // namespace gpbo
