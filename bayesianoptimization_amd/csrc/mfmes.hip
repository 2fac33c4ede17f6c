// Multi-fidelity max-value entropy search (the GIBBON lower bound; Moss, Leslie & Rayson 2021; qLowerBoundMaxValueEntropy with a
// fidelity column at q = 1) over the resident candidates (gfx950): gpmf_mes_argbest's values.  include/gpmf.h has the formulas, the
// order of every sum and the conventions; mf_plan.h the tiling.  Per candidate row z (fidelity s = z[fid_col]) and its twin z' at
// the target fidelity:
//   u = W k*(z), u' = W k*(z')        q = |u|^2, q' = |u'|^2, x = u . u', m' = alpha . k*(z')
//   ys = (1 / (2 S)) sum_s log1p(-rho^2 (1 - r2(gamma_s))) / (cost0 + cost1 s)
// the posterior COVARIANCE of f(z) and f(z') is the new quantity: a bilinear form no posterior pass produces.
// Compiled with -ffp-contract=off, as jes.hip (the fmas below are written out).
//
// One kernel, mf_pair_kernel, and the selection behind it:
//   ownership   a workgroup of eight waves owns 32 candidates — 32 PAIRS — and walks ALL row chunks of W itself, rows the outer loop,
//               k-stages the inner, the k loop of a chunk stopping at the chunk's last row (W is lower triangular).  The three sums
//               of a candidate therefore never leave the workgroup: no partials in memory, no finalize launch, bits independent of M.
//   generation  thread = (candidate c, train point p) of the stage: 32 x 16 = 512.  The squared distance over the d - 1 shared
//               coordinates is formed ONCE — the fidelity column is zero in the candidates' LDS image and in the staged train points,
//               so its term of the chain is an exact 0 — then the two fidelity terms are added, the kernel function runs twice, and
//               both values go to LDS in B-fragment order.  m' is accumulated here, in the last chunk's walk (the one that sees every
//               train point).  Generation is repeated per row chunk; the stage ahead is generated into registers in front of the
//               current stage's MFMAs and stored behind them: one barrier per stage.
//   product     fragment 2 g + e of a stage holds member e (0: z, 1: z') of candidate group g, so the accumulators of u and u' of
//               the same (row, candidate) sit in the same lane, register for register.  A wave owns the 16-row tiles w and 15 - w of
//               the chunk (equal work in the diagonal block); each W fragment it loads (packed W, one k-pair per 16-byte load, a
//               stage ahead) feeds four MFMAs: both members of both groups.
//   sums        behind a chunk's walk u u, u' u' and u u' are lane-local fmas into six running sums per lane (two groups x three),
//               chunk after chunk; behind the last chunk the four row groups of a wave by two xor shuffles, the eight waves in wave
//               order through LDS.
//   score       thread c < 32 turns its sums into vl, vg, cv, rho^2; all 512 threads evaluate the (candidate, sample) terms — r2 is
//               jes.hip's device function (jes_r2.h), lanes diverge over its ranges — into LDS; thread c adds its S terms in order,
//               applies the cost and the conventions and stores ys and the optional parts.
//   select      the existing arg-best / top-k over ctx->ys (acq_kernels.hip), from the entry point.
// Candidates from M on in the last tile read the zero rows of the padded scaled image and are not written.
#include "gpbo_internal.h"
#include "jes_r2.h"
#include "mf_plan.h"

#include <cmath>

namespace gpbo {

typedef double mf_d4 __attribute__((ext_vector_type(4)));

struct MfArgs {
  const double* Wp;       // packed W (fit_bodies.h: pack_w_elem)
  const double* Xs;       // [NP][DP] scaled train points
  const double* alpha;    // [NP], zero from N on
  const double* ls;       // length scales
  const double* P;        // [>= round_up(M, 128)][DP] the scaled candidates, zero rows from M on
  const double* Xc;       // [M][d] the raw candidates (the cost reads the fidelity in parameter units)
  const double* y_star;   // [S] device
  double* ys;
  double* rho;            // [M] or null
  double* mu_t;
  double* sd_t;
  int64_t M;
  int NP, d, fid, S;
  double fid_target, cost0, cost1, amplitude, lambda, y_mean, y_std;
};

template <int DP, int KERNEL>
__global__ __launch_bounds__(MF_WAVES * 64, 2) void mf_pair_kernel(const MfArgs a) {
  constexpr int NT = MF_WAVES * 64;
  constexpr int XP = DP + MF_XS_PAD;
  constexpr int NE = (MF_BK * DP + NT - 1) / NT;      // staged coordinates per thread and stage
  __shared__ __attribute__((aligned(16))) double lds[mf_lds_doubles(DP)];
  double* Ks = lds;                               // [2][4 k-steps][4 fragments][64]
  double* Xl = lds + mf_lds_frags();              // [DP][32], the fidelity column zero
  double* xs = Xl + DP * MF_CANDS;                // [2][16][XP], the fidelity column zero
  double* xf = xs + 2 * MF_BK * XP;               // [2][16] the train points' fidelity coordinates
  double* al = xf + 2 * MF_BK;                    // [2][16] their alphas
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * MF_CANDS;
  const int NP = a.NP, fid = a.fid;
  // generation role: candidate gc, train point gp of the stage
  const int gc = lane & 31, gp = 2 * wave + (lane >> 5);
  const double tf = a.fid_target / a.ls[fid];                   // the target fidelity, scaled as prescale_elem scales a coordinate
  const double zf = a.P[(m0 + gc) * DP + fid];
  for (int e = tid; e < MF_CANDS * DP; e += NT) {
    const int cnd = e / DP, t = e - cnd * DP;
    const double v = a.P[m0 * DP + e];
    Xl[t * MF_CANDS + cnd] = t == fid ? 0.0 : v;
  }

  double pv[NE], av = 0.0;
  auto pts_load = [&](const int st) {
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int e = tid + NT * j;
      pv[j] = e < MF_BK * DP ? a.Xs[(int64_t)st * MF_BK * DP + e] : 0.0;
    }
    if (tid < MF_BK) av = a.alpha[st * MF_BK + tid];
  };
  auto pts_store = [&](const int st) {
    const int slot = st & 1;
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int e = tid + NT * j;
      if (e < MF_BK * DP) {
        const int row = e / DP, t = e - row * DP;
        xs[(slot * MF_BK + row) * XP + t] = t == fid ? 0.0 : pv[j];
        if (t == fid) xf[slot * MF_BK + row] = pv[j];
      }
    }
    if (tid < MF_BK) al[slot * MF_BK + tid] = av;
  };
  double mu_acc = 0.0;
  // k(z, X_p) and k(z', X_p) of stage st from one shared distance; with_mean: alpha_p k' into this thread's partial mean
  auto gen = [&](const int st, const bool with_mean, double& kz, double& kt) {
    const int slot = st & 1;
    const double* xr = xs + (slot * MF_BK + gp) * XP;
    double d2 = 0.0;
    if constexpr (DP <= 8) {
#pragma unroll
      for (int t = 0; t < DP; ++t) {
        const double df = Xl[t * MF_CANDS + gc] - xr[t];
        d2 = fma(df, df, d2);
      }
    } else {
#pragma unroll 1
      for (int tb = 0; tb < DP; tb += 8) {
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
          const double df = Xl[(tb + tt) * MF_CANDS + gc] - xr[tb + tt];
          d2 = fma(df, df, d2);
        }
      }
    }
    const double f = xf[slot * MF_BK + gp];
    const double dz = zf - f, dt = tf - f;
    kz = gpbo_kernel_value<KERNEL>(fma(dz, dz, d2));
    kt = gpbo_kernel_value<KERNEL>(fma(dt, dt, d2));
    if (with_mean) mu_acc = fma(kt, al[slot * MF_BK + gp], mu_acc);
  };
  auto gen_store = [&](const int st, const double kz, const double kt) {
    double* dst = Ks + (((st & 1) * 4 + (gp >> 2)) * 4 + 2 * (gc >> 4)) * 64 + (gp & 3) * 16 + (gc & 15);
    dst[0] = kz;
    dst[64] = kt;
  };

  const int nchunks = mf_chunks(NP);
  const int64_t pairs = NP / 8;
  const double2* Wp2 = reinterpret_cast<const double2*>(a.Wp);
  double sq[2] = {0.0, 0.0}, st2[2] = {0.0, 0.0}, sx[2] = {0.0, 0.0};      // per group: u u, u' u', u u' of this lane's rows

  for (int r = 0; r < nchunks; ++r) {
    const int n_stages = mf_chunk_stages(NP, r);
    const bool last = r == nchunks - 1;
    const int tA = mf_tile_a(r, wave), tB = mf_tile_b(r, wave);
    // A tile beyond NP (a ragged last chunk) is never read: its loads go to tile 0, which every k-pair of the walk holds, it rides
    // along with the other tile's stages, and its accumulators are dropped below.  tA < tB, so tile A beyond NP means both are.
    const bool actA = tA * 16 < NP, actB = tB * 16 < NP;
    // the last stage each tile multiplies; -1: none
    const int sA = actA ? mf_tile_last_stage(tA, n_stages) : -1;
    const int sB = actB ? mf_tile_last_stage(tB, n_stages) : sA;
    const int eA = actA ? tA : 0, eB = actB ? tB : 0;
    const double2* wpA = Wp2 + ((int64_t)(eA >> 1) * pairs * 2 + (eA & 1)) * 64 + lane;
    const double2* wpB = Wp2 + ((int64_t)(eB >> 1) * pairs * 2 + (eB & 1)) * 64 + lane;
    mf_d4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int f = 0; f < 4; ++f) acc[t][f] = mf_d4{0.0, 0.0, 0.0, 0.0};
    // W fragments, [tile]: w0 the stage's first k-pair (8 columns), w1 its second; elements x / y a k-pair's two k-steps.  Each is
    // refilled right behind its last use: w1 at the top of its stage, w0 for the next stage behind this stage's first k-pair.
    double2 w0[2] = {}, w1[2] = {};
    auto load_w = [&](const int kpair, const bool ta, const bool tb, double2 (&w)[2]) {
      if (ta) w[0] = wpA[(int64_t)kpair * 128];
      if (tb) w[1] = wpB[(int64_t)kpair * 128];
    };
    auto mma_pair = [&](const double* kb, const int pp, const double2 (&w)[2], auto mode) {
      constexpr int MODE = decltype(mode)::value;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const double a0 = e ? w[0].y : w[0].x;
        const double a1 = e ? w[1].y : w[1].x;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const double b = kb[((2 * pp + e) * 4 + f) * 64];
          if constexpr (MODE == 2) acc[0][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][f], 0, 0, 0);
          acc[1][f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][f], 0, 0, 0);
        }
      }
    };

    pts_load(0);
    pts_store(0);
    if (n_stages > 1) {
      pts_load(1);
      pts_store(1);
    }
    load_w(0, 0 <= sA, 0 <= sB, w0);
    __syncthreads();      // the stages' points (and, the first time, the candidates' image) are whole
    {
      double kz, kt;
      gen(0, last, kz, kt);
      gen_store(0, kz, kt);
    }
    __syncthreads();
    // One stage.  MODE 2: both tiles multiply, 1: only the later tile, 0: none (the wave only generates) — compile-time, so that
    // the accumulators keep their registers across the three loops below.
    auto stage = [&](const int st, auto mode) {
      constexpr int MODE = decltype(mode)::value;
      const bool more = st + 1 < n_stages, more2 = st + 2 < n_stages;
      double kz = 0.0, kt = 0.0;
      if (more2) pts_load(st + 2);
      if constexpr (MODE > 0) load_w(2 * st + 1, MODE == 2, true, w1);
      if (more) gen(st + 1, last, kz, kt);
      if constexpr (MODE > 0) {
        const double* kb = Ks + (st & 1) * 1024 + lane;
        mma_pair(kb, 0, w0, mode);
        load_w(2 * st + 2, st + 1 <= sA, st + 1 <= sB, w0);
        mma_pair(kb, 1, w1, mode);
      }
      if (more) gen_store(st + 1, kz, kt);
      if (more2) pts_store(st + 2);
      __syncthreads();
    };
    int st = 0;
    for (; st <= sA; ++st) stage(st, std::integral_constant<int, 2>{});
    for (; st <= sB; ++st) stage(st, std::integral_constant<int, 1>{});
    for (; st < n_stages; ++st) stage(st, std::integral_constant<int, 0>{});
    // the chunk's rows into the lane's sums: tile w, then tile 15 - w, the accumulator registers in order; a tile beyond NP adds nothing
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (!(t == 0 ? actA : actB)) continue;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const double u = acc[t][2 * g][rr], v = acc[t][2 * g + 1][rr];
          sq[g] = fma(u, u, sq[g]);
          st2[g] = fma(v, v, st2[g]);
          sx[g] = fma(u, v, sx[g]);
        }
      }
  }

  // behind the walk's last barrier the LDS is the score's
  double* red = lds;                                      // [3][8 waves][32]
  double* mured = red + 3 * MF_WAVES * MF_CANDS;          // [16 points of a stage][32]
  double* scal = mured + MF_BK * MF_CANDS;                // [6][32]: rho^2, m', sqrt(vg), cv, vg, vo (NaN: a bad candidate)
  double* terms = scal + 6 * MF_CANDS;                    // [32][65]
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    double v0 = sq[g], v1 = st2[g], v2 = sx[g];
    v0 = v0 + __shfl_xor(v0, 16);
    v1 = v1 + __shfl_xor(v1, 16);
    v2 = v2 + __shfl_xor(v2, 16);
    v0 = v0 + __shfl_xor(v0, 32);
    v1 = v1 + __shfl_xor(v1, 32);
    v2 = v2 + __shfl_xor(v2, 32);
    if (lane < 16) {
      red[(0 * MF_WAVES + wave) * MF_CANDS + 16 * g + lane] = v0;
      red[(1 * MF_WAVES + wave) * MF_CANDS + 16 * g + lane] = v1;
      red[(2 * MF_WAVES + wave) * MF_CANDS + 16 * g + lane] = v2;
    }
  }
  mured[gp * MF_CANDS + gc] = mu_acc;
  __syncthreads();
  const int64_t mrow = m0 + (tid & 31) < a.M ? m0 + (tid & 31) : a.M - 1;
  if (tid < MF_CANDS) {
    double q = red[tid], qt = red[MF_WAVES * MF_CANDS + tid], x = red[2 * MF_WAVES * MF_CANDS + tid], mp = mured[tid];
#pragma unroll
    for (int w = 1; w < MF_WAVES; ++w) {
      q = q + red[w * MF_CANDS + tid];
      qt = qt + red[(MF_WAVES + w) * MF_CANDS + tid];
      x = x + red[(2 * MF_WAVES + w) * MF_CANDS + tid];
    }
#pragma unroll
    for (int p = 1; p < MF_BK; ++p) mp = mp + mured[p * MF_CANDS + tid];
    double t1 = 1.0 - q, t2 = 1.0 - qt;
    t1 = t1 < 0.0 ? 0.0 : t1;      // a NaN stays
    t2 = t2 < 0.0 ? 0.0 : t2;
    const double vl = a.amplitude * t1, vg = a.amplitude * t2;
    const double dfid = a.P[mrow * DP + fid] - tf;
    const double kap = gpbo_kernel_value<KERNEL>(dfid * dfid);
    const double cv = a.amplitude * (kap - x);
    const double vo = vl + a.lambda;
    double rho2 = 0.0;
    if (vo > 0.0 && vg > 0.0) {
      rho2 = (cv * cv) / (vo * vg);
      rho2 = rho2 > 1.0 ? 1.0 : rho2;
    }
    const bool bad = q != q || qt != qt || x != x || mp != mp || kap != kap;
    scal[tid] = rho2;
    scal[MF_CANDS + tid] = mp;
    scal[2 * MF_CANDS + tid] = sqrt(vg);
    scal[3 * MF_CANDS + tid] = cv;
    scal[4 * MF_CANDS + tid] = vg;
    scal[5 * MF_CANDS + tid] = bad ? __builtin_nan("") : vo;      // vo is finite wherever q is
  }
  __syncthreads();
  {
    // thread (c, j): candidate c, samples j, j + 16, ...
    const int c = tid & 31;
    const double rho2 = scal[c], mp = scal[MF_CANDS + c], sdg = scal[2 * MF_CANDS + c];
    for (int s = tid >> 5; s < a.S; s += NT / MF_CANDS) {
      double term = 0.0;
      if (rho2 > 0.0 && sdg > 0.0) {
        const double gam = ((a.y_star[s] - a.y_mean) / a.y_std - mp) / sdg;
        term = log1p(-(rho2 * (1.0 - jes_r2_dev(gam))));
      }
      terms[c * (MF_MAX_SAMPLES + 1) + s] = term;
    }
  }
  __syncthreads();
  if (tid >= MF_CANDS || m0 + tid >= a.M) return;
  const int64_t i = m0 + tid;
  double total = 0.0;
  for (int s = 0; s < a.S; ++s) total = total + terms[tid * (MF_MAX_SAMPLES + 1) + s];
  const double rho2 = scal[tid], mp = scal[MF_CANDS + tid], sdg = scal[2 * MF_CANDS + tid], cv = scal[3 * MF_CANDS + tid];
  const double vg = scal[4 * MF_CANDS + tid], vo = scal[5 * MF_CANDS + tid];
  const bool bad = vo != vo;
  const double nan = __builtin_nan("");
  double info = -(total / (2.0 * (double)a.S));
  if (vg == 0.0 || vo == 0.0) info = 0.0;
  const double cost = a.cost0 + a.cost1 * a.Xc[i * a.d + fid];
  double ys = -info / cost;
  if (bad || !(cost > 0.0) || !(cost < INFINITY)) ys = nan;
  a.ys[i] = ys;
  if (a.rho) a.rho[i] = bad ? nan : copysign(sqrt(rho2), cv);
  if (a.mu_t) a.mu_t[i] = a.y_std * mp + a.y_mean;
  if (a.sd_t) a.sd_t[i] = a.y_std * sdg;
}

// debug build: an event before and after each stage of the last call (gpmf_debug_stage_ms); the product records nothing
static inline void mf_mark(gpbo_ctx* ctx, int i) {
#ifdef GPBO_DEBUG
  StageClock& c = ctx->mf_clock;
  if (!c.ev[i]) (void)hipEventCreate(&c.ev[i]);
  (void)hipEventRecord(c.ev[i], ctx->stream);
  c.used = (i == c.n - 1);
#else
  (void)ctx; (void)i;
#endif
}

int launch_mf_values(gpbo_ctx* ctx, const Model& m, int64_t M, int fid_col, double fid_target, double cost0, double cost1,
                     const double* y_star, int S, double y_mean, double y_std, bool parts) {
  const int d = m.d, DP = m.DP;
  int rc;
  static_assert(MF_PARTS_AT == MF_MAX_SAMPLES, "the parts lie behind the sampled maxima");
  // the call's workspace: y_star [64] | rho [M] | mu_t [M] | sd_t [M] (the parts only when one is asked for)
  if ((rc = ensure(ctx, &ctx->mf, &ctx->cap_mf, MF_MAX_SAMPLES + (parts ? 3 * M : 0)))) return rc;
  GPBO_HIP(ctx, hipMemcpyAsync(ctx->mf, y_star, (size_t)S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const int64_t Mp = round_up(M, POST_CANDS);
  if ((rc = ensure(ctx, &ctx->Xcs, &ctx->cap_Xcs, Mp * DP))) return rc;
  if ((rc = launch_prescale(ctx, ctx->Xc, M, d, DP, m.ls, ctx->Xcs, Mp))) return rc;
  if ((rc = ensure(ctx, &ctx->ys, &ctx->cap_ys, M))) return rc;
  const int64_t blocks = mf_blocks(M);
  if (blocks > 0x7fffffffLL) GPBO_FAIL(ctx, GPBO_ERR_UNSUPPORTED, "mf_mes_argbest: grid too large; shard the candidates");
  MfArgs a{};
  a.Wp = m.Wp; a.Xs = m.Xs; a.alpha = m.alpha; a.ls = m.ls; a.P = ctx->Xcs; a.Xc = ctx->Xc; a.y_star = ctx->mf; a.ys = ctx->ys;
  double* out = ctx->mf + MF_MAX_SAMPLES;
  if (parts) { a.rho = out; a.mu_t = out + M; a.sd_t = out + 2 * M; }
  a.M = M; a.NP = (int)m.NP; a.d = d; a.fid = fid_col; a.S = S;
  a.fid_target = fid_target; a.cost0 = cost0; a.cost1 = cost1; a.amplitude = m.amplitude; a.lambda = m.amplitude * m.noise;
  a.y_mean = y_mean; a.y_std = y_std;
  mf_mark(ctx, 0);
  rc = with_dp_kernel(ctx, DP, m.kernel, [&](auto dp, auto k) {
    mf_pair_kernel<decltype(dp)::value, decltype(k)::value><<<dim3((unsigned)blocks), dim3(MF_WAVES * 64), 0, ctx->stream>>>(a);
    GPBO_HIP(ctx, hipGetLastError());
    return GPBO_OK;
  });
  if (rc) return rc;
  mf_mark(ctx, 1);      // stage 2, the selection, is the caller's; it records event 2 behind it (mf_mark_end)
  return GPBO_OK;
}

void mf_mark_end(gpbo_ctx* ctx) { mf_mark(ctx, 2); }

}  // namespace gpbo
